"""Numpy restatement of the connected-component contracts of include/ucsa_hip.h
(ucsa_voxel_components, ucsa_graph_components, ucsa_component_sizes) and of the
two utilities built on them (utils/tsdf_fusion.remove_small_components,
utils/mesh_fusion.filter_mesh_components).  A label is the smallest index of
its component, so the GPU outputs must match these byte for byte.

The labelling is vectorised hooking and pointer jumping over an edge list: every
round hooks the larger of the two roots of each edge under the smaller
(np.minimum.at) and then flattens the forest completely; it ends when the two
ends of every edge share a root."""
import numpy as np

I32 = np.int32


def edge_components(n, ea, eb):
    """labels int64 [n] of the graph on 0..n-1 with edges (ea[i], eb[i])"""
    parent = np.arange(n, dtype=np.int64)
    ea = np.asarray(ea, np.int64)
    eb = np.asarray(eb, np.int64)
    while ea.size:
        pa, pb = parent[ea], parent[eb]
        differ = pa != pb
        if not differ.any():
            break
        ea, eb, pa, pb = ea[differ], eb[differ], pa[differ], pb[differ]
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
    return parent


def earlier_offsets(connectivity):
    """the neighbours that come before a voxel in the order of the linear index"""
    if connectivity == 6:
        return [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    if connectivity == 26:
        cube = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
        return [o for o in cube if o < (0, 0, 0)]
    raise ValueError("connectivity must be 6 or 26")


def lattice_edges(mask, connectivity):
    m = np.asarray(mask) != 0
    nx, ny, nz = m.shape
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    ea, eb = [], []
    for dx, dy, dz in earlier_offsets(connectivity):
        def cut(d, n):
            # (own range, neighbour's range) along one axis
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (ox, px), (oy, py), (oz, pz) = cut(dx, nx), cut(dy, ny), cut(dz, nz)
        both = m[ox, oy, oz] & m[px, py, pz]
        ea.append(idx[ox, oy, oz][both])
        eb.append(idx[px, py, pz][both])
    return np.concatenate(ea), np.concatenate(eb)


def voxel_components(mask, connectivity=26):
    """int32 [nx,ny,nz]: the smallest linear index of the component, -1 off the mask"""
    m = np.asarray(mask) != 0
    ea, eb = lattice_edges(m, connectivity)
    lab = edge_components(m.size, ea, eb).reshape(m.shape)
    return np.where(m, lab, -1).astype(I32)


def graph_components(offsets, neighbours):
    """int32 [V]: the smallest vertex index of the component"""
    offsets = np.asarray(offsets, np.int64)
    V = offsets.size - 1
    src = np.repeat(np.arange(V, dtype=np.int64), np.diff(offsets))
    return edge_components(V, src, np.asarray(neighbours, np.int64)).astype(I32)


def component_sizes(labels):
    """int32 of labels' shape: how many elements carry labels[x]; 0 where it is < 0"""
    lab = np.asarray(labels)
    flat = lab.reshape(-1).astype(np.int64)
    ok = flat >= 0
    counts = np.bincount(flat[ok], minlength=max(flat.size, 1))
    return np.where(ok, counts[np.where(ok, flat, 0)], 0).astype(I32).reshape(lab.shape)


def band_mask(vol, min_weight=1):
    with np.errstate(invalid="ignore"):
        return (vol["weight"] >= np.float32(min_weight)) & (vol["tsdf"] < np.float32(1.0))


def _stats(sizes_of_roots, small, what):
    return {"components": int(sizes_of_roots.size), "removed_components": int(small.sum()),
            what: int(sizes_of_roots[small].sum()),
            "largest": int(sizes_of_roots.max()) if sizes_of_roots.size else 0}


def remove_small_components(vol, min_voxels, connectivity=26, min_weight=1):
    """in place on a dict of numpy arrays (tsdf, weight, rgb or None) -> statistics"""
    band = band_mask(vol, min_weight)
    lab = voxel_components(band, connectivity)
    sizes = component_sizes(lab)
    roots = lab.reshape(-1) == np.arange(lab.size)
    rs = sizes.reshape(-1)[roots]
    st = _stats(rs, rs < int(min_voxels), "removed_voxels")
    if int(min_voxels) > 1:
        drop = band & (sizes < int(min_voxels))
        vol["tsdf"][drop] = 1.0
        vol["weight"][drop] = 0.0
        if vol.get("rgb") is not None:
            vol["rgb"][drop] = 0.0
    return st


def mesh_adjacency(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    key = np.unique(np.concatenate([a * V + b, b * V + a]))
    src = key // max(V, 1)
    offsets = np.zeros(V + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(src, minlength=V))
    return offsets.astype(I32), (key - src * V).astype(I32)


def filter_mesh_components(mesh, min_vertices=0, keep_largest=None):
    """-> (new dict, statistics), the rule of utils/mesh_fusion.filter_mesh_components"""
    V = int(np.asarray(mesh["verts"]).shape[0])
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    lab = graph_components(*mesh_adjacency(faces, V)).astype(np.int64)
    sizes = component_sizes(lab)
    roots = np.flatnonzero(lab == np.arange(V))
    rs = sizes[roots]
    keep_root = rs >= int(min_vertices)
    if keep_largest is not None:
        order = sorted(range(roots.size), key=lambda i: (-int(rs[i]), int(roots[i])))
        top = np.zeros(roots.size, bool)
        top[order[:int(keep_largest)]] = True
        keep_root &= top
    keep_v = np.isin(lab, roots[keep_root])
    new_id = np.cumsum(keep_v) - 1
    keep_f = keep_v[faces].all(1) if faces.size else np.zeros(0, bool)
    out = dict(mesh)
    for k in ("verts", "normals", "rgb", "labels"):
        if mesh.get(k) is not None:
            out[k] = np.asarray(mesh[k])[keep_v]
    out["faces"] = new_id[faces[keep_f]].astype(I32).reshape(-1, 3)
    out["vertex_index"], out["face_index"] = np.flatnonzero(keep_v), np.flatnonzero(keep_f)
    return out, _stats(rs, ~keep_root, "removed_vertices")


def serpentine(dims):
    """a one-voxel-wide path that sweeps the whole lattice plane by plane: along
    z in every other row of every other x-plane, the rows joined at alternating
    ends, the planes joined through one voxel of the plane in between.  One
    component at either connectivity."""
    nx, ny, nz = dims
    m = np.zeros(dims, bool)
    end = 0                                        # the z at which the path stands
    for i in range(0, nx, 2):
        rows = list(range(0, ny, 2))
        if (i // 2) % 2:
            rows.reverse()
        for n, j in enumerate(rows):
            m[i, j, :] = True
            end = nz - 1 - end                     # the row is walked to its other end
            if n + 1 < len(rows):
                m[i, (j + rows[n + 1]) // 2, end] = True
        if i + 2 < nx:
            m[i + 1, rows[-1], end] = True
    return m
