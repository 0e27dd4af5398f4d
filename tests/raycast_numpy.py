"""numpy restatement of the ray cast against a triangle mesh
(csrc/tri_ray.h, csrc/mesh_raycast.hip: ucsa_raycast_mesh, ucsa_mesh_occluded;
ops.raycast.raycast_mesh, ops.raycast.mesh_occluded).

``raycast_mesh`` / ``mesh_occluded`` are the definition: plain brute force over
all faces with the intersection of ``intersect``, float32 and float64 exactly
as include/ucsa_hip.h states them, nothing fused.  They know nothing of cells,
so the result cannot depend on the cell size, the grid's origin or the order of
the rays.

``raycast_grid`` is a model of the kernel's traversal over
``surface_numpy.triangle_grid``: the slab supercover along the ray's major
axis, layer by layer in ray order, with the kernel's float32 expressions for
the layer range, a layer's parameter interval, the minor ranges, the skipped
layers and the stop rule.  tests/test_raycast_cpu.py holds it to the brute
force byte for byte, which proves slack and stop rule before any GPU run.
Inside a layer the kernel takes candidates one by one and the model takes them
all at once; the best candidate is the minimum of (t, face) over the visited
set, which no order and no repeated evaluation changes."""
import numpy as np

from tests import surface_numpy as SN
from tests.nearest_numpy import F, NONE, _f32

D = np.float64
K = F(2.0 ** -20)          # the box clause (docs/DESIGN_NOTEBOOK.md, section RC)
KT = F(2.0 ** -17)         # the traversal's slack: 8 K
FLT_MAX = np.finfo(F).max


def _sel(P, k):
    """component k (an int array) of the triple of arrays P, as the kernel selects it"""
    return np.where(k == 0, P[0], np.where(k == 1, P[1], P[2]))


def major_axis(d):
    """kz = argmax |d|, the first on ties; d a triple of arrays"""
    a0, a1, a2 = np.abs(d[0]), np.abs(d[1]), np.abs(d[2])
    kz = np.where(a1 > a0, 1, 0)
    return np.where(a2 > np.maximum(a0, a1), 2, kz)


def valid_rays(O, Dr):
    return np.isfinite(O).all(-1) & np.isfinite(Dr).all(-1) & (Dr != 0).any(-1)


def intersect(O, Dr, kz, A, B, C, tmin, tmax):
    """One (ray, face) pair per element of the broadcast: O, Dr, A, B, C triples
    of float32 arrays, kz the ray's major axis, tmin / tmax float32 ->
    (hit bool, t float32, U, V, W, det float64).  Steps 2 to 7 of the contract."""
    with np.errstate(all="ignore"):
        kx, ky = (kz + 1) % 3, (kz + 2) % 3
        okx, oky, okz = _sel(O, kx), _sel(O, ky), _sel(O, kz)
        dkz = _sel(Dr, kz)
        Sx, Sy = _sel(Dr, kx) / dkz, _sel(Dr, ky) / dkz
        sheared = []
        for P in (A, B, C):
            px, py, pz = _sel(P, kx) - okx, _sel(P, ky) - oky, _sel(P, kz) - okz
            X, Y = px - Sx * pz, py - Sy * pz
            assert X.dtype == F and Y.dtype == F and pz.dtype == F
            sheared.append((X.astype(D), Y.astype(D), pz.astype(D)))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = sheared
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        det = (U + V) + W
        inside = ((((U >= 0) & (V >= 0) & (W >= 0)) | ((U <= 0) & (V <= 0) & (W <= 0)))
                  & (det != 0))
        t = (((U * Az + V * Bz) + W * Cz) / det / dkz.astype(D)).astype(F)
        hit = inside & np.isfinite(t) & (tmin <= t) & (t <= tmax)
        for a in range(3):
            td = t * Dr[a]
            p = O[a] + td
            mn = np.minimum(np.minimum(A[a], B[a]), C[a])
            mx = np.maximum(np.maximum(A[a], B[a]), C[a])
            S = K * ((np.abs(O[a]) + np.abs(td)) + np.maximum(np.abs(mn), np.abs(mx)))
            assert p.dtype == F and S.dtype == F
            hit = hit & (mn - S <= p) & (p <= mx + S)
    return hit, t, U, V, W, det


def _bary(U, V, W, det):
    with np.errstate(all="ignore"):
        return np.stack([U / det, V / det, W / det], -1).astype(F)


def _ranges(t_min, t_max, n):
    tmin = np.ascontiguousarray(np.broadcast_to(np.asarray(t_min, F), (n,)))
    tmax = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, F), (n,)))
    return tmin, tmax


def raycast_mesh(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, chunk_pairs=1 << 18):
    """-> (face int32 [N], t float32 [N], bary float32 [N,3]): the hit with the
    smallest t, among equal t the smallest face index; a miss: -1, +inf, zeros."""
    V, Fc, O, Dr = _f32(verts), SN._faces(faces), _f32(origins), _f32(dirs)
    n = O.shape[0]
    tmin, tmax = _ranges(t_min, t_max, n)
    face = np.full(n, -1, np.int32)
    t = np.full(n, np.inf, F)
    bary = np.zeros((n, 3), F)
    fid = np.nonzero(SN.valid_faces(V, Fc))[0]
    if fid.size == 0 or n == 0:
        return face, t, bary
    A, B, C = (tuple(V[Fc[fid, c], a][None, :] for a in range(3)) for c in range(3))
    ok_ray = valid_rays(O, Dr)
    step = max(1, chunk_pairs // fid.size)
    for s in range(0, n, step):
        o = tuple(O[s:s + step, a, None] for a in range(3))
        d = tuple(Dr[s:s + step, a, None] for a in range(3))
        hit, tt, U, Vv, W, det = intersect(o, d, major_axis(d), A, B, C,
                                           tmin[s:s + step, None], tmax[s:s + step, None])
        hit = hit & ok_ray[s:s + step, None]
        j = np.argmin(np.where(hit, tt, F(np.inf)), axis=1)          # the first minimum
        rows = np.arange(hit.shape[0])
        h = hit[rows, j]
        face[s:s + step] = np.where(h, fid[j], -1)
        t[s:s + step] = np.where(h, tt[rows, j], F(np.inf))
        bary[s:s + step] = np.where(h[:, None],
                                    _bary(U[rows, j], Vv[rows, j], W[rows, j], det[rows, j]), F(0))
    return face, t, bary


def mesh_occluded(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf):
    """-> uint8 [N]: whether any face is hit in the range"""
    return (raycast_mesh(verts, faces, origins, dirs, t_min, t_max)[0] >= 0).astype(np.uint8)


# ---- the traversal ----------------------------------------------------------
def _cell(x, g, h, dim):
    """pg_cell((x - g) / h, dim) -> int64"""
    with np.errstate(all="ignore"):
        u = (x - g) / h
        u = np.minimum(np.maximum(np.where(np.isnan(u), F(0), u), F(0)), (dim - 1).astype(F))
    return np.floor(u).astype(np.int64)


def raycast_grid(verts, faces, origins, dirs, t_min=0.0, t_max=np.inf, cell=None, origin=None,
                 any_hit=False, stats=None):
    """The kernels' traversal over ``triangle_grid``'s records -> (face, t, bary),
    or the any-hit byte with ``any_hit`` (that walk stops at its first hit)."""
    g = SN.triangle_grid(verts, faces, cell, origin)
    O, Dr = _f32(origins), _f32(dirs)
    n = O.shape[0]
    tmin, tmax = _ranges(t_min, t_max, n)
    rec, offsets, P = g["records"], g["offsets"].astype(np.int64), g["n_pairs"]
    go, h, dims = g["origin"], g["cell"], np.asarray(g["dims"], np.int64)
    best = np.full(n, np.inf, F)
    bidx = np.full(n, NONE, np.uint32)
    bary = np.zeros((n, 3), F)
    visited = 0
    if n and P:
        with np.errstate(all="ignore"):
            o, d = tuple(O[:, a] for a in range(3)), tuple(Dr[:, a] for a in range(3))
            kz = major_axis(d)
            kx, ky = (kz + 1) % 3, (kz + 2) % 3
            top = go + dims.astype(F) * h
            S3 = tuple(KT * ((np.abs(o[a]) + np.abs(go[a])) + np.abs(top[a])) for a in range(3))
            g3, t3 = tuple(go[a] + 0 * o[a] for a in range(3)), tuple(top[a] + 0 * o[a] for a in range(3))
            n3 = tuple(dims[a] + 0 * kz for a in range(3))
            wide = ~(np.isfinite(S3[0]) & np.isfinite(S3[1]) & np.isfinite(S3[2]))
            oz, dz, gz, Sz, nz = _sel(o, kz), _sel(d, kz), _sel(g3, kz), _sel(S3, kz), _sel(n3, kz)
            tlo, thi = np.fmax(tmin, -FLT_MAX), np.fmin(tmax, FLT_MAX)
            za, zb = oz + tlo * dz, oz + thi * dz
            ia = _cell(np.minimum(za, zb) - Sz, gz, h, nz)
            ib = _cell(np.maximum(za, zb) + Sz, gz, h, nz)
            ia, ib = np.where(wide, 0, ia), np.where(wide, nz - 1, ib)
            active = valid_rays(O, Dr)
            fwd = dz > 0
        s = 0
        while active.any():
            R = np.nonzero(active)[0]
            i = np.where(fwd[R], ia[R] + s, ib[R] - s)
            s += 1
            off = (i < ia[R]) | (i > ib[R])
            active[R[off]] = False
            R, i = R[~off], i[~off]
            with np.errstate(all="ignore"):
                zl = gz[R] + i.astype(F) * h
                zh = gz[R] + (i + 1).astype(F) * h
                tA = ((zl - Sz[R]) - oz[R]) / dz[R]
                tB = ((zh + Sz[R]) - oz[R]) / dz[R]
                t0, t1 = np.minimum(tA, tB), np.maximum(tA, tB)
                stop = (best[R] < t0) | (t0 > thi[R])                 # no later layer can win
                tc0, tc1 = np.fmax(t0, tlo[R]), np.fmin(t1, thi[R])
                skip = tc0 > tc1
                lo_c, hi_c = {}, {}
                for name, k in (("x", kx[R]), ("y", ky[R])):
                    om = _sel(tuple(c[R] for c in o), k)
                    dm = _sel(tuple(c[R] for c in d), k)
                    gm = _sel(tuple(c[R] for c in g3), k)
                    tm = _sel(tuple(c[R] for c in t3), k)
                    Sm = _sel(tuple(c[R] for c in S3), k)
                    nm = _sel(tuple(c[R] for c in n3), k)
                    x0, x1 = om + tc0 * dm, om + tc1 * dm
                    xl, xh = np.minimum(x0, x1) - Sm, np.maximum(x0, x1) + Sm
                    skip = skip | (~wide[R] & ((xh < gm) | (xl > tm + Sm)))
                    lo_c[name] = np.where(wide[R], 0, _cell(xl, gm, h, nm))
                    hi_c[name] = np.where(wide[R], nm - 1, _cell(xh, gm, h, nm))
            active[R[stop]] = False
            go_on = ~stop & ~skip
            R, i = R[go_on], i[go_on]
            if R.size == 0:
                continue
            c0 = np.zeros((R.size, 3), np.int64)
            c1 = np.zeros((R.size, 3), np.int64)
            rows = np.arange(R.size)
            c0[rows, kz[R]], c1[rows, kz[R]] = i, i
            c0[rows, kx[R]], c1[rows, kx[R]] = lo_c["x"][go_on], hi_c["x"][go_on]
            c0[rows, ky[R]], c1[rows, ky[R]] = lo_c["y"][go_on], hi_c["y"][go_on]
            assert (c0 <= c1).all() and (c0 >= 0).all() and (c1 < dims[None, :]).all()
            ext = c1 - c0 + 1
            visited += int(ext.prod(1).sum())
            ncol = ext[:, 0] * ext[:, 1]                                 # runs along z
            r_of = np.repeat(rows, ncol)
            kcol = np.arange(int(ncol.sum())) - np.repeat(np.cumsum(ncol) - ncol, ncol)
            x = c0[r_of, 0] + kcol // ext[r_of, 1]
            y = c0[r_of, 1] + kcol % ext[r_of, 1]
            row = (x * dims[1] + y) * dims[2]
            bs = np.clip(offsets[row + c0[r_of, 2]], 0, P)
            es = np.clip(offsets[row + c1[r_of, 2] + 1], 0, P)
            cnt = np.maximum(es - bs, 0)
            if cnt.sum() == 0:
                continue
            qi = np.repeat(R[r_of], cnt)
            k = np.repeat(bs - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
            A, B, C = (tuple(rec[k, 4 * c + a] for a in range(3)) for c in range(3))
            j = np.ascontiguousarray(rec[k, 3]).view(np.uint32)
            hit, tt, U, Vv, W, det = intersect(tuple(c[qi] for c in o), tuple(c[qi] for c in d),
                                               kz[qi], A, B, C, tmin[qi], tmax[qi])
            take = hit & ((tt < best[qi]) | ((tt == best[qi]) & (j < bidx[qi])))
            qi, tt, j, bb = qi[take], tt[take], j[take], _bary(U[take], Vv[take], W[take], det[take])
            first = np.lexsort((j, tt, qi))
            qi, tt, j, bb = qi[first], tt[first], j[first], bb[first]
            head = np.ones(qi.size, bool)
            head[1:] = qi[1:] != qi[:-1]
            best[qi[head]], bidx[qi[head]], bary[qi[head]] = tt[head], j[head], bb[head]
            if any_hit:
                active[qi[head]] = False
    if stats is not None:
        stats["cells_visited"] = visited
        stats["cells"] = int(np.prod(dims))
    hit = bidx != NONE
    if any_hit:
        return hit.astype(np.uint8)
    face = np.where(hit, bidx, 0).astype(np.int64).astype(np.int32)
    face[~hit] = -1
    return face, np.where(hit, best, F(np.inf)).astype(F), bary
