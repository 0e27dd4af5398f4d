"""numpy restatement of the signed distance to a triangle mesh
(csrc/mesh_sdf.hip: ucsa_face_unit_normals, ucsa_normal_runs, ucsa_mesh_sign,
ucsa_mesh_tsdf; ops.mesh_pseudonormals, ops.signed_distance, ops.mesh_tsdf).

Every operation is rounded to float32 and nothing is fused.  The sums over a
vertex's corners and over an edge's half-edges are plain loops in the order of
the items; the search is tests/surface_numpy.py's brute force over all faces,
so a result cannot depend on a cell grid; ``mesh_tsdf`` is that brute force over
every lattice point.  The corner angles are an input of the contract (the op's
own are fed back in the byte comparisons); ``corner_angles`` is the same formula
in float32 numpy for the tests that have no GPU."""
import numpy as np

from tests.nearest_numpy import F, _f32
from tests.surface_numpy import _faces, closest, dot, nearest_triangle, valid_faces

# region (the nearest-triangle section's order, from 0; 6 = interior) -> feature
# 0 face, 1 AB, 2 BC, 3 CA, 4 A, 5 B, 6 C
FEATURE_OF_REGION = np.array([4, 5, 1, 6, 3, 2, 0], np.int32)


def face_unit_normals(verts, faces):
    """ucsa_face_unit_normals -> float32 [F,3]"""
    V, Fc = _f32(verts), _faces(faces)
    out = np.zeros((Fc.shape[0], 3), F)
    ok = valid_faces(V, Fc)
    with np.errstate(all="ignore"):
        for f in np.nonzero(ok)[0]:
            A, B, C = V[Fc[f, 0]], V[Fc[f, 1]], V[Fc[f, 2]]
            e1, e2 = B - A, C - A
            n = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                 e1[0] * e2[1] - e1[1] * e2[0])
            l = np.sqrt(dot(n, n))
            if l > 0 and np.isfinite(l):
                out[f] = (n[0] / l, n[1] / l, n[2] / l)
    assert out.dtype == F
    return out


def corner_angles(verts, faces):
    """atan2(|u x w|, u . w) of the two edges leaving each corner, float32 [F,3],
    0 for an invalid face (what ops.mesh_pseudonormals computes in torch)"""
    V, Fc = _f32(verts), _faces(faces)
    out = np.zeros((Fc.shape[0], 3), F)
    ok = valid_faces(V, Fc)
    with np.errstate(all="ignore"):
        for f in np.nonzero(ok)[0]:
            P = V[Fc[f]]
            for k in range(3):
                u, w = P[(k + 1) % 3] - P[k], P[(k + 2) % 3] - P[k]
                c = (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2],
                     u[0] * w[1] - u[1] * w[0])
                a = np.arctan2(np.sqrt(dot(c, c)), dot(u, w))
                out[f, k] = a if np.isfinite(a) else F(0)
    return out


def normal_runs(items, run_first, n_runs, weight, unit_normal):
    """ucsa_normal_runs -> float32 [n_runs,3]: per run a sequential sum, in the
    order of the items, of weight * unit normal (the product, then the sum)"""
    items = np.asarray(items, np.int32)
    run_first = np.asarray(run_first, np.int32)
    unit = np.asarray(unit_normal, F).reshape(-1, 3)
    nf = unit.shape[0]
    out = np.zeros((n_runs, 3), F)
    with np.errstate(all="ignore"):
        for r in range(n_runs):
            b = max(int(run_first[r]), 0)
            e = min(int(run_first[r + 1]), items.size)
            acc = [F(0), F(0), F(0)]
            for pos in range(b, e):
                it = int(items[pos])
                if not 0 <= it < 3 * nf:
                    continue
                w = F(1) if weight is None else F(weight[it])
                for c in range(3):
                    acc[c] = F(acc[c] + F(w * unit[it // 3, c]))
            out[r] = acc
    return out


def vertex_runs(V, Fc):
    """the valid corners 3f+k by vertex, ties by 3f+k -> (items, run_first [V+1])"""
    ok = np.repeat(valid_faces(V, Fc), 3)
    items = np.arange(3 * Fc.shape[0], dtype=np.int32)[ok]
    vid = Fc.reshape(-1)[ok].astype(np.int64)
    order = np.argsort(vid, kind="stable")
    first = np.searchsorted(vid[order], np.arange(V.shape[0] + 1), side="left").astype(np.int32)
    return items[order], first


def edge_runs(V, Fc):
    """the valid half-edges 3f+k (corner k -> corner (k+1)%3) by undirected edge,
    ties by 3f+k -> (items, run_first [E+1], run of every position)"""
    ok = np.repeat(valid_faces(V, Fc), 3)
    items = np.arange(3 * Fc.shape[0], dtype=np.int32)[ok]
    a = Fc.reshape(-1)[ok].astype(np.int64)
    b = Fc[:, [1, 2, 0]].reshape(-1)[ok].astype(np.int64)
    key = np.minimum(a, b) * max(V.shape[0], 1) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    head = np.ones(skey.size, bool)
    head[1:] = skey[1:] != skey[:-1]
    first = np.append(np.nonzero(head)[0], skey.size).astype(np.int32)
    return items[order], first, np.cumsum(head) - 1


def pseudonormals(verts, faces, corner_angle):
    """ops.mesh_pseudonormals with the corner angles given -> dict of float32
    arrays: unit_normal [F,3], vertex_normal [V,3], edge_normal [F,3,3]"""
    V, Fc = _f32(verts), _faces(faces)
    nf = Fc.shape[0]
    unit = face_unit_normals(V, Fc)
    ang = np.ascontiguousarray(np.asarray(corner_angle, F).reshape(-1))
    assert ang.size == 3 * nf
    items, first = vertex_runs(V, Fc)
    vertex = normal_runs(items, first, V.shape[0], ang, unit)
    items, first, run = edge_runs(V, Fc)
    sums = normal_runs(items, first, first.size - 1, None, unit)
    edge = np.zeros((3 * nf, 3), F)
    edge[items] = sums[run]
    return {"unit_normal": unit, "vertex_normal": vertex, "edge_normal": edge.reshape(nf, 3, 3)}


def closest_feature(a, b, c):
    """surface_numpy.closest plus the region that decided (first match in the
    written order; 6 = interior) and the closest point p, the query at the origin
    -> (v, w, dist2, region, p)"""
    sub = lambda x, y: (x[0] - y[0], x[1] - y[1], x[2] - y[2])
    neg = lambda x: (-x[0], -x[1], -x[2])
    v, w, dist2 = closest(a, b, c)
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
        region = np.select(conds, [0, 1, 2, 3, 4, 5], 6)
        p = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
    return v, w, dist2, region, p


def mesh_sign(verts, faces, normals, queries, face):
    """ucsa_mesh_sign -> (sdf float32 [Q], feature int32 [Q])"""
    V, Fc, Q = _f32(verts), _faces(faces), _f32(queries)
    face = np.asarray(face, np.int32)
    nq, nf = Q.shape[0], Fc.shape[0]
    sdf = np.full(nq, np.inf, F)
    feature = np.full(nq, -1, np.int32)
    un, vn, en = (np.asarray(normals[k], F) for k in ("unit_normal", "vertex_normal",
                                                      "edge_normal"))
    good = (face >= 0) & (face < nf)
    good[good] = valid_faces(V, Fc)[face[good]]
    idx = np.nonzero(good)[0]
    if idx.size == 0:
        return sdf, feature
    f, q = face[idx], Q[idx]
    with np.errstate(all="ignore"):
        a, b, c = (tuple(V[Fc[f, s], t] - q[:, t] for t in range(3)) for s in range(3))
        _, _, dist2, region, p = closest_feature(a, b, c)
        ft = FEATURE_OF_REGION[region]
        N = un[f]                                                   # feature 0
        N = np.where((ft >= 1)[:, None] & (ft <= 3)[:, None], en[f, np.clip(ft - 1, 0, 2)], N)
        N = np.where((ft >= 4)[:, None], vn[Fc[f, np.clip(ft - 4, 0, 2)]], N)
        s = -dot(p, (N[:, 0], N[:, 1], N[:, 2]))
        d = np.sqrt(dist2)
        out = np.where(s < 0, -d, d)
    assert out.dtype == F
    sdf[idx] = out
    feature[idx] = ft
    return sdf, feature


def signed_distance(verts, faces, normals, queries, max_dist):
    """ops.signed_distance as brute force -> (sdf, face, dist2, bary, feature)"""
    face, dist2, bary = nearest_triangle(verts, faces, queries, max_dist)
    sdf, feature = mesh_sign(verts, faces, normals, queries, face)
    return sdf, face, dist2, bary, feature


def lattice_points(dims, origin, spacing):
    """origin[a] + (float)i_a * spacing[a] in float32, z fastest -> [nx*ny*nz,3]"""
    ax = [F(origin[a]) + np.arange(dims[a]).astype(F) * F(spacing[a]) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    assert g.dtype == F
    return g


def mesh_tsdf(tsdf, weight, origin, spacing, verts, faces, normals, trunc, weight_value):
    """ucsa_mesh_tsdf as brute force over the lattice -> (tsdf, weight), copies
    with the band written and every other voxel as it was"""
    tsdf = np.array(tsdf, F)
    weight = np.array(weight, F)
    pts = lattice_points(tsdf.shape, origin, spacing)
    sdf, face, _, _, _ = signed_distance(verts, faces, normals, pts, trunc)
    hit = face >= 0
    with np.errstate(all="ignore"):
        t = sdf / F(trunc)
    t = np.where(t < -1, F(-1), t)
    t = np.where(t > 1, F(1), t)
    tsdf.reshape(-1)[hit] = t[hit]
    weight.reshape(-1)[hit] = F(weight_value)
    return tsdf, weight


# ---- the meshes of tests/test_sdf_cpu.py and tests/test_gpu_sdf.py ------------
def _outward(V, Fc):
    """orient the faces of a convex solid away from its centroid (float64)"""
    V64 = np.asarray(V, np.float64)
    Fc = np.array(Fc, np.int32)
    ctr = V64.mean(0)
    for f in range(Fc.shape[0]):
        A, B, C = V64[Fc[f]]
        if np.dot(np.cross(B - A, C - A), (A + B + C) / 3 - ctr) < 0:
            Fc[f] = Fc[f, ::-1]
    return Fc


def tetrahedron():
    """regular, corners at (+-1, +-1, +-1), outward -> (V, F, inside(q float64))"""
    V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
    Fc = _outward(V, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    return V, Fc, lambda q: _inside_convex(V, Fc, q)


def cube():
    """a box of 12 faces, outward"""
    lo, hi = np.array([-1.0, -0.75, -0.5]), np.array([1.0, 0.75, 0.5])
    V = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]]
                  for i in range(2) for j in range(2) for k in range(2)], F)
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    Fc = _outward(V, [t for a, b, c, d in quads for t in ([a, b, c], [a, c, d])])
    return V, Fc, lambda q: np.all((q > lo) & (q < hi), axis=-1)


def l_prism():
    """an L-shaped prism of 20 faces (not convex), outward; inside = a union of
    two boxes"""
    poly = np.array([[0, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2]], np.float64)
    shift = np.array([-1.0, -1.0, -0.5])
    V = np.array([[x, y, z] for z in (0.0, 1.0) for x, y in poly]) + shift
    tris = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]]
    Fc = [[a, c, b] for a, b, c in tris] + [[6 + a, 6 + b, 6 + c] for a, b, c in tris]
    for i in range(6):
        j = (i + 1) % 6
        Fc += [[i, j, 6 + j], [i, 6 + j, 6 + i]]
    boxes = [(np.array([0.0, 0, 0]) + shift, np.array([2.0, 1, 1]) + shift),
             (np.array([0.0, 0, 0]) + shift, np.array([1.0, 2, 1]) + shift)]

    def inside(q):
        return np.any([np.all((q > lo) & (q < hi), axis=-1) for lo, hi in boxes], axis=0)
    return V.astype(F), np.array(Fc, np.int32), inside


def _inside_convex(V, Fc, q):
    V64 = np.asarray(V, np.float64)
    ins = np.ones(q.shape[0], bool)
    for f in Fc:
        A, B, C = V64[f]
        ins &= (q - A) @ np.cross(B - A, C - A) < 0
    return ins


def open_patch():
    """two triangles sharing an edge, in the plane z = 0, normal +z"""
    V = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def fan(n=9):
    """n faces around one apex above a regular n-gon (open at the bottom)"""
    t = 2 * np.pi * np.arange(n) / n
    V = np.concatenate([[[0.1, -0.05, 0.7]], np.stack([np.cos(t), np.sin(t), 0 * t], 1)]).astype(F)
    Fc = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return V, Fc


def broken_mesh():
    """the cube plus a degenerate face, a face with an index out of range, a
    negative index, a face at a NaN vertex and one at an infinite vertex"""
    V, Fc, _ = cube()
    V = np.concatenate([V, [[np.nan, 0, 0], [np.inf, 1, 1], [2, 2, 2]]]).astype(F)
    extra = [[0, 0, 3], [0, 1, 11], [-1, 2, 3], [8, 1, 2], [3, 9, 5], [10, 10, 10]]
    return V, np.concatenate([Fc[:5], extra, Fc[5:]]).astype(np.int32)
