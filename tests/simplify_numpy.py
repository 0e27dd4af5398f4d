"""numpy restatement of mesh simplification by vertex clustering
(csrc/mesh_simplify.hip: ucsa_vertex_cluster_keys, ucsa_cluster_reduce,
ucsa_cluster_faces; ops.simplify_mesh; utils/mesh_fusion.py: simplify_mesh,
pool_label_table).

Plain loops.  Every float sum is taken scalar by scalar in float32, in the order
the contract names (a cluster's members by label, then by original index);
nothing here is a vectorised sum whose order numpy chooses.  Element-wise
float32 arithmetic (the cell of a coordinate) is vectorised: it has no order."""
import math

import numpy as np

F = np.float32
MAX_DIM = 1 << 18
NO_CLUSTER = np.int64(0x7FFFFFFFFFFFFFFF)


def grid_of(verts, cell, origin=None):
    """-> (origin float32 [3], cell float32, dims): the minimum corner of the
    finite vertices unless given, dims = floor(extent / cell) + 1 in float64 on
    float32 corners."""
    v = np.asarray(verts, F).reshape(-1, 3)
    cell = F(cell)
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError("cell must be positive and finite")
    fin = v[np.isfinite(v).all(1)]
    lo = fin.min(0) if fin.size else np.zeros(3, F)
    hi = fin.max(0) if fin.size else np.zeros(3, F)
    if origin is not None:
        lo = np.asarray(origin, F).reshape(3)
        if not np.isfinite(lo).all():
            raise ValueError("origin must be finite")
    dims = tuple(int(math.floor(max(float(b) - float(a), 0.0) / float(cell))) + 1
                 for a, b in zip(lo, hi))
    if max(dims) > MAX_DIM:
        raise ValueError("an axis needs more than 2^18 cells: raise cell")
    return lo.astype(F), cell, dims


def cluster_keys(verts, origin, cell, dims, labels=None):
    """-> int64 [V]: (((ix << 18 | iy) << 18 | iz) << 8) | label, the cell being
    floor(clamp((p - origin) / cell, 0, dim - 1)) in float32; a non-finite vertex
    gets INT64_MAX."""
    v = np.asarray(verts, F).reshape(-1, 3)
    o, c = np.asarray(origin, F), F(cell)
    with np.errstate(all="ignore"):
        t = (v - o[None, :]) / c
    assert t.dtype == F
    top = np.asarray([d - 1 for d in dims], F)
    t = np.where(np.isnan(t), F(0), t)                       # fmaxf(NaN, 0) = 0
    idx = np.floor(np.minimum(np.maximum(t, F(0)), top[None, :])).astype(np.int64)
    lab = np.zeros(v.shape[0], np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    key = (((idx[:, 0] << 18 | idx[:, 1]) << 18 | idx[:, 2]) << 8) | lab
    return np.where(np.isfinite(v).all(1), key, NO_CLUSTER).astype(np.int64)


def cluster_offsets(keys, split_labels):
    """-> (order int32 [V]: the stable sort of the keys; first int32 [K+1]: where
    each cluster starts in it).  A cluster is a cell, or a (cell, label) pair."""
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    sk = keys[order]
    n_fin = int((sk != NO_CLUSTER).sum())
    ident = sk[:n_fin] if split_labels else sk[:n_fin] >> 8
    first = [k for k in range(n_fin) if k == 0 or ident[k] != ident[k - 1]] + [n_fin]
    if n_fin == 0:
        first = [0]
    return order, np.asarray(first, np.int32)


def cluster_reduce(verts, order, first, normals=None, rgb=None, labels=None):
    """-> dict: verts float32 [K,3], count int32 [K] and, for the inputs given,
    normals float32 [K,3], rgb uint8 [K,3], labels uint8 [K]."""
    v = np.asarray(verts, F).reshape(-1, 3)
    K = len(first) - 1
    out = {"verts": np.zeros((K, 3), F), "count": np.zeros(K, np.int32)}
    if normals is not None:
        nrm = np.asarray(normals, F).reshape(-1, 3)
        out["normals"] = np.zeros((K, 3), F)
    if rgb is not None:
        col = np.asarray(rgb, np.uint8).reshape(-1, 3)
        out["rgb"] = np.zeros((K, 3), np.uint8)
    if labels is not None:
        lab = np.asarray(labels).astype(np.int64)
        out["labels"] = np.zeros(K, np.uint8)
    with np.errstate(all="ignore"):
        for c in range(K):
            mem = [int(order[k]) for k in range(int(first[c]), int(first[c + 1]))]
            n = len(mem)
            out["count"][c] = n
            x0 = v[mem[0]]
            for a in range(3):
                s = F(0)
                for m in mem:
                    s = F(s + F(v[m, a] - x0[a]))
                out["verts"][c, a] = x0[a] if n == 1 else F(x0[a] + F(s / F(n)))
            if normals is not None:
                s = [F(0), F(0), F(0)]
                for m in mem:
                    for a in range(3):
                        s[a] = F(s[a] + nrm[m, a])
                ln = F(np.sqrt(F(F(F(s[0] * s[0]) + F(s[1] * s[1])) + F(s[2] * s[2]))))
                for a in range(3):
                    out["normals"][c, a] = F(s[a] / ln) if ln > 0 else F(0)
            if rgb is not None:
                for a in range(3):
                    tot = sum(int(col[m, a]) for m in mem)
                    out["rgb"][c, a] = (2 * tot + n) // (2 * n)
            if labels is not None:
                best, best_run, run, prev = 0, 0, 0, -1
                for m in mem:
                    l = int(lab[m])
                    run = run + 1 if l == prev else 1
                    prev = l
                    if l > 0 and run > best_run:
                        best, best_run = l, run
                out["labels"][c] = best
    return out


def cluster_faces(faces, vertex_map):
    """-> (tri int32 [F,3], keep uint8 [F]): each corner through ``vertex_map``;
    a corner index outside [0, V), a corner mapped to -1 or two corners on one
    cluster drop the face (its row is -1 -1 -1); else the triple rotated so that
    its smallest index comes first."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    vm = np.asarray(vertex_map, np.int32)
    V = vm.shape[0]
    tri = np.full((f.shape[0], 3), -1, np.int32)
    keep = np.zeros(f.shape[0], np.uint8)
    for i in range(f.shape[0]):
        a, b, c = (int(x) for x in f[i])
        if min(a, b, c) < 0 or max(a, b, c) >= V:
            continue
        a, b, c = int(vm[a]), int(vm[b]), int(vm[c])
        if min(a, b, c) < 0 or a == b or b == c or a == c:
            continue
        if b < a and b < c:
            a, b, c = b, c, a
        elif c < a and c < b:
            a, b, c = c, a, b
        tri[i] = (a, b, c)
        keep[i] = 1
    return tri, keep


def simplify_mesh(verts, faces, cell, normals=None, rgb=None, labels=None, split_labels=False,
                  origin=None):
    """The whole of ops.simplify_mesh -> dict of numpy arrays (see its docstring)."""
    v = np.asarray(verts, F).reshape(-1, 3)
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    if labels is not None:
        lab = np.asarray(labels)
        if lab.size and (lab.min() < 0 or lab.max() > 255):
            raise ValueError("labels must be in 0..255")
    o, c, dims = grid_of(v, cell, origin)
    keys = cluster_keys(v, o, c, dims, labels)
    order, first = cluster_offsets(keys, split_labels)
    K = len(first) - 1
    out = cluster_reduce(v, order, first, normals, rgb, labels)
    vmap = np.full(v.shape[0], -1, np.int32)
    for k in range(K):
        for j in range(int(first[k]), int(first[k + 1])):
            vmap[order[j]] = k
    tri, keep = cluster_faces(f, vmap)
    seen, rows, index = set(), [], []
    for i in range(f.shape[0]):
        t = tuple(int(x) for x in tri[i])
        if keep[i] and t not in seen:
            seen.add(t)
            rows.append(t)
            index.append(i)
    out["faces"] = np.asarray(rows, np.int32).reshape(-1, 3)
    out["face_index"] = np.asarray(index, np.int32)
    out["vertex_map"] = vmap
    out["origin"], out["cell"], out["dims"] = tuple(float(x) for x in o), float(c), dims
    out["degenerate"] = int(f.shape[0] - int(keep.sum()))
    out["duplicate"] = int(keep.sum()) - len(rows)
    out["keys"], out["order"], out["first"], out["tri"], out["keep"] = keys, order, first, tri, keep
    return out


def pool_label_table(votes, vertex_map, n_out):
    """rows of a [V, C+1] uint64 table added into the rows ``vertex_map`` names,
    modulo 2^64; a row mapped to -1 is skipped"""
    t = np.asarray(votes).view(np.uint64)
    out = np.zeros((int(n_out), t.shape[1]), np.uint64)
    with np.errstate(over="ignore"):
        for i in range(t.shape[0]):
            k = int(vertex_map[i])
            if k >= 0:
                for c in range(t.shape[1]):
                    out[k, c] = out[k, c] + t[i, c]
    return out.view(np.int64)
