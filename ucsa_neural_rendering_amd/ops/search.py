"""Spatial search: point and triangle grids, nearest point and triangle, mesh
voxelization, pseudonormals and the signed distance to a mesh."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import (_finite_box, _gpu, _mesh, _non_negative, _origin_spacing, _points3,
                    _positive, _ptr, _stream, volume_lattice)


# ---------------------------------------------------------------------------
# nearest point within a radius (cell grid)
# ---------------------------------------------------------------------------
POINT_GRID_MAX_CELLS = 1 << 24


def _cell_sort(keys, ncells: int):
    """int32 cell ``keys`` -> (``order`` int64: by key, ties by position;
    ``offsets`` int32 [ncells+1]: where each cell starts in that order)"""
    order = torch.sort(keys, stable=True).indices
    offsets = torch.searchsorted(keys[order].contiguous(),
                                 torch.arange(ncells + 1, dtype=torch.int32, device=keys.device)
                                 ).to(torch.int32)
    return order, offsets


def _search_args(grid, maker: str, payload: str, count: str, cols: int, queries, max_dist,
                 sort_queries: bool):
    """What ``nearest_point`` and ``nearest_triangle`` do before their library
    call: the queries, the grid dict of ops.``maker`` (its ``payload`` float32
    [grid[``count``], ``cols``]) and ``max_dist`` checked, and the queries' cell
    order -> (q, payload, offsets, n, origin, cell, dims, q_order, nq, max_dist)
    as the library takes them."""
    q = _points3(queries, "queries")
    try:
        pay, offsets = grid[payload], grid["offsets"]
        origin, cell, dims, n = grid["origin"], float(grid["cell"]), grid["dims"], int(grid[count])
    except (TypeError, KeyError):
        raise _lib.UcsaError(f"grid must be the dict of ops.{maker}")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    _gpu(pay, f"grid: {payload}", torch.float32, (n, cols), device=q.device, fixed=True)
    _gpu(offsets, "grid: offsets", torch.int32, numel=ncells + 1, device=q.device, fixed=True)
    max_dist = _positive(max_dist, "max_dist")
    nq = int(q.shape[0])
    org, dm = fvec(origin), (C.c_uint32 * 3)(*[int(d) for d in dims])
    q_order = None
    if sort_queries and nq and n:
        keys = torch.empty(nq, dtype=torch.int32, device=q.device)
        check(lib().ucsa_point_cell_keys(_ptr(q), nq, org, cell, dm, 0, _ptr(keys), _stream()),
              "ucsa_point_cell_keys")
        q_order = torch.sort(keys, stable=True).indices.to(torch.int32)
    return q, pay, offsets, n, org, cell, dm, q_order, nq, max_dist


def _grid_shape(lo, hi, n, cell):
    """origin, cell and dims from the finite points' box: host arithmetic in
    float64 on float32 corners.  The choice changes time only, never a result."""
    ext = [float(b) - float(a) for a, b in zip(lo, hi)]
    big = max(ext)
    if cell is None:
        pad = [e + max(big, 1e-30) * 1e-3 for e in ext]
        cell = (pad[0] * pad[1] * pad[2] / max(n, 1)) ** (1.0 / 3.0)
    cell = _positive(cell, "cell")
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    cell = f32(max(cell, big / 1024.0, 1e-30))
    # more than 64 cells per point buy nothing and cost an offset each
    cap = min(POINT_GRID_MAX_CELLS, max(4096, 64 * n))
    while True:
        dims = tuple(int(math.floor(e / cell)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cap:
            return cell, dims
        cell = f32(cell * 1.25)


def point_grid(points, cell=None):
    """A uniform cell grid over ``points`` [N,3] (float32 on the GPU) for
    ``nearest_point`` -> dict: ``origin`` (3 floats) and ``dims`` (3 ints) from
    the finite points' bounding box, ``cell``, ``offsets`` int32 [cells+1],
    ``order`` int32 [N] (the points by cell, ties by index; non-finite points
    last), ``sorted_points`` float32 [N,4] (x, y, z and the bits of the original
    index in w), ``n``.  The default cell is the cube root of the padded box's
    volume per point, at least 1/1024 of the largest extent, and raised until
    the grid has at most min(2^24, max(4096, 64 N)) cells; an explicit ``cell``
    is raised the same way.  The cell changes time only, never a result.  The
    keys are a kernel (ucsa_point_cell_keys), the sort is torch on the device."""
    pts = _points3(points, "points")
    n = int(pts.shape[0])
    dev = pts.device
    lo, hi = _finite_box(pts, torch.isfinite(pts).all(1))
    cell, dims = _grid_shape(lo, hi, n, cell)
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().ucsa_point_cell_keys(_ptr(pts), n, fvec(lo), cell, (C.c_uint32 * 3)(*dims), 1,
                                     _ptr(keys), _stream()), "ucsa_point_cell_keys")
    order64, offsets = _cell_sort(keys, dims[0] * dims[1] * dims[2])
    order = order64.to(torch.int32)
    packed = torch.empty((n, 4), dtype=torch.int32, device=dev)
    packed[:, :3] = pts[order64].view(torch.int32)
    packed[:, 3] = order
    return {"origin": tuple(float(v) for v in lo), "cell": cell, "dims": dims,
            "offsets": offsets, "order": order, "sorted_points": packed.view(torch.float32),
            "n": n}


def nearest_point(grid, queries, max_dist: float, sort_queries: bool = True):
    """For each of ``queries`` [Q,3] (float32 on the GPU) the nearest point of
    ``grid`` (``point_grid``'s dict) within ``max_dist`` -> (``index`` int32 [Q],
    ``dist2`` float32 [Q]) on the device: the original index of the nearest
    point and the squared distance, -1 and +inf where no point lies within
    ``max_dist`` (inclusive).  Among equally near points the smallest index
    wins; a non-finite point or query matches nothing.  ``max_dist`` is required
    and finite: an unbounded search is not offered, and a query with nothing
    near walks every cell within ``max_dist``, so passing the scene's diagonal
    costs what a brute-force search costs for such queries.  ``sort_queries``
    hands the queries to the kernel in cell order, so that a wave's lanes walk
    the same cells; it changes time only.  Contract of ucsa_nearest_point
    (include/ucsa_hip.h)."""
    q, sp, offsets, n, org, cell, dm, q_order, nq, max_dist = _search_args(
        grid, "point_grid", "sorted_points", "n", 4, queries, max_dist, sort_queries)
    index = torch.empty(nq, dtype=torch.int32, device=q.device)
    dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    check(lib().ucsa_nearest_point(_ptr(sp) if n else None, _ptr(offsets) if n else None, n, org,
                                   cell, dm, _ptr(q), _ptr(q_order), nq, max_dist, _ptr(index),
                                   _ptr(dist2), _stream()), "ucsa_nearest_point")
    return index, dist2


TRIANGLE_GRID_MAX_PAIRS = 0x7FFFFFFF


def triangle_grid(verts, faces, cell=None):
    """A uniform cell grid over the faces of a triangle mesh (``verts`` [V,3]
    float32, ``faces`` [F,3] int32, on the GPU) for ``nearest_triangle`` -> dict:
    ``origin`` (3 floats) and ``dims`` (3 ints) from the finite vertices'
    bounding box, ``cell``, ``offsets`` int32 [cells+1], ``records`` float32
    [P,12] (per (cell, face) pair, by cell and faces ascending inside a cell:
    A.xyz and the bits of the face index, B.xyz and 0, C.xyz and 0),
    ``n_pairs`` = P, ``n_faces``.  A face is registered in every cell of the box
    between its corners' cells; a face with a corner index outside [0, V) or a
    non-finite corner is registered nowhere.  The default cell is the (lower)
    median over the valid faces of the longest side of the face's box, at least
    1/1024 of the largest extent; it is raised by a quarter while the grid has
    more than min(2^24, max(4096, 64 F)) cells or more than max(65536, 32 F)
    pairs, and an explicit ``cell`` is raised the same way.  The cell changes
    time only, never a result.  Counts and pairs are kernels
    (ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs); scan, sort and
    packing are torch on the device."""
    v, f = _mesh(verts, faces)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if cell is not None:
        _positive(cell, "cell")
    dev = v.device
    fin = torch.isfinite(v).all(1)
    lo, hi = _finite_box(v, fin)
    ext = [float(b) - float(a) for a, b in zip(lo, hi)]
    big = max(ext)
    if cell is None:
        ok = ((f >= 0) & (f < nv)).all(1) if nv else torch.zeros(nf, dtype=torch.bool, device=dev)
        if nv and nf:
            ok &= fin[f.clamp(0, nv - 1).long()].all(1)
        if nf and bool(ok.any()):
            corners = v[f[ok].long()]                                   # [F',3,3]
            side = (corners.max(1).values - corners.min(1).values).max(1).values
            cell = float(torch.sort(side).values[(side.numel() - 1) // 2])
        else:
            cell = big
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    cell = f32(max(float(cell), big / 1024.0, 1e-30))
    cell_cap = min(POINT_GRID_MAX_CELLS, max(4096, 64 * nf))
    pair_cap = max(65536, 32 * nf)
    org = fvec(lo)
    counts = torch.empty(nf, dtype=torch.int32, device=dev)
    while True:
        dims = tuple(int(math.floor(e / cell)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cell_cap:
            dm = (C.c_uint32 * 3)(*dims)
            check(lib().ucsa_triangle_cell_counts(_ptr(v), nv, _ptr(f), nf, org, cell, dm,
                                                  _ptr(counts), _stream()),
                  "ucsa_triangle_cell_counts")
            n_pairs = int(counts.sum(dtype=torch.int64)) if nf else 0
            if n_pairs <= pair_cap:
                break
        cell = f32(cell * 1.25)
    if n_pairs > TRIANGLE_GRID_MAX_PAIRS:
        raise _lib.UcsaError(f"{n_pairs} (cell, face) pairs: at most 2^31-1")
    first = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).to(torch.int32)
    keys = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    pair_face = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    check(lib().ucsa_triangle_cell_pairs(_ptr(v), nv, _ptr(f), nf, org, cell, dm, _ptr(first),
                                         n_pairs, _ptr(keys), _ptr(pair_face), _stream()),
          "ucsa_triangle_cell_pairs")
    order, offsets = _cell_sort(keys, dims[0] * dims[1] * dims[2])
    sf = pair_face[order]
    rec = torch.zeros((n_pairs, 12), dtype=torch.int32, device=dev)
    if n_pairs:
        tri = f[sf.long()].long()
        for c in range(3):
            rec[:, 4 * c:4 * c + 3] = v[tri[:, c]].view(torch.int32)
        rec[:, 3] = sf
    return {"origin": tuple(float(x) for x in lo), "cell": cell, "dims": dims,
            "offsets": offsets, "records": rec.view(torch.float32), "n_pairs": n_pairs,
            "n_faces": nf}


def nearest_triangle(grid, queries, max_dist: float, sort_queries: bool = True):
    """For each of ``queries`` [Q,3] (float32 on the GPU) the nearest point on the
    faces of ``grid`` (``triangle_grid``'s dict) within ``max_dist`` -> (``face``
    int32 [Q], ``dist2`` float32 [Q], ``bary`` float32 [Q,3]) on the device: the
    face, the squared distance to its closest point and that point's
    barycentric weights of the face's three corners; -1, +inf and a zero row
    where no face lies within ``max_dist`` (inclusive).  Among equally near
    faces the smallest index wins; an invalid face or a non-finite query matches
    nothing.  ``max_dist`` is required and finite, as in ``nearest_point``, and
    costs the same: a query with nothing near walks every cell within it.
    ``sort_queries`` hands the queries to the kernel in cell order; it changes
    time only.  Contract of ucsa_nearest_triangle (include/ucsa_hip.h)."""
    q, rec, offsets, n, org, cell, dm, q_order, nq, max_dist = _search_args(
        grid, "triangle_grid", "records", "n_pairs", 12, queries, max_dist, sort_queries)
    face = torch.empty(nq, dtype=torch.int32, device=q.device)
    dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    bary = torch.empty((nq, 3), dtype=torch.float32, device=q.device)
    check(lib().ucsa_nearest_triangle(_ptr(rec) if n else None, _ptr(offsets) if n else None, n,
                                      org, cell, dm, _ptr(q), _ptr(q_order), nq, max_dist,
                                      _ptr(face), _ptr(dist2), _ptr(bary), _stream()),
          "ucsa_nearest_triangle")
    return face, dist2, bary


# ---------------------------------------------------------------------------
# mesh voxelization (the cells of a lattice or of the cascade grid a mesh meets)
# ---------------------------------------------------------------------------
VOXELIZE_LATTICE, VOXELIZE_CASCADE = 0, 1


def _voxelize(what, verts, faces, family, dims, origin, spacing, bound, cascade, dilate, out):
    pts, fc = _mesh(verts, faces, 0x7FFFFFFF // cascade, any_integer=True)
    dev = pts.device
    V, F = int(pts.shape[0]), int(fc.shape[0])
    dilate = _non_negative(dilate, f"{what}: dilate")
    nx, ny, nz = dims
    shape = (nx, ny, nz) if family == VOXELIZE_LATTICE else (cascade, nx, ny, nz)
    if out is None:
        mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        mask = _gpu(out, "out", torch.uint8, shape, device=dev, fixed=True)
    o3 = fvec(origin) if origin is not None else None
    s3 = fvec(spacing) if spacing is not None else None
    geo = (_ptr(pts) if V else None, V, _ptr(fc) if F else None, F, family, nx, ny, nz, o3, s3,
           bound, cascade, dilate)
    items = F * cascade
    ws_bytes = int(lib().ucsa_mesh_voxelize_workspace_bytes(F, cascade))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev) if items else None
    count = torch.empty(items, dtype=torch.int32, device=dev) if items else None
    check(lib().ucsa_mesh_voxelize_count(*geo, _ptr(count), _ptr(ws), ws_bytes, _stream()),
          "ucsa_mesh_voxelize_count")
    first, total = None, 0
    if items:
        first = torch.zeros(items + 1, dtype=torch.int64, device=dev)
        first[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(first[items])
    check(lib().ucsa_mesh_voxelize_fill(*geo, _ptr(first), total, 0 if out is None else 1,
                                        _ptr(mask), mask.numel(), _ptr(ws), ws_bytes, _stream()),
          "ucsa_mesh_voxelize_fill")
    return mask


def voxelize_mesh(verts, faces, dims, origin, spacing, dilate: float = 0.0, out=None):
    """The voxels of a lattice that a triangle mesh passes through: uint8
    [nx,ny,nz] on the mesh's device, 1 = some face meets the voxel's box.  The
    lattice is ``tsdf_volume``'s: voxel (i,j,k) is the box of side ``spacing``
    (a number or 3) centred on origin + (i,j,k)*spacing, grown by ``dilate``
    (scene units) on every side; the mask can index a volume's arrays and go to
    ``voxel_components``.  ``verts`` float32 [V,3], ``faces`` an integer tensor
    [F,3] with indices in [0,V), both on the GPU; a face with a non-finite
    corner marks nothing, a segment or a point marks the voxels it touches.
    ``out`` (uint8 [nx,ny,nz], contiguous) accumulates: met voxels are set to 1
    and every other byte is left alone, so any split of the faces over calls
    gives the bytes of one call.  F = 0 gives an all-zero mask.  Contract of
    ucsa_mesh_voxelize_count / ucsa_mesh_voxelize_fill (include/ucsa_hip.h):
    conservative in float32 (a touching pair is never lost), a pure OR, the
    same bytes every run and for every face order.  Reads back the face index
    range (validation) and, between the two kernels, the column total."""
    try:
        dims = tuple(int(d) for d in dims)
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"voxelize_mesh: dims must be 3 integers, got {dims!r}")
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > 0x7FFFFFFF:
        raise _lib.UcsaError(f"voxelize_mesh: dims must be 3 integers >= 1 with at most 2^31-1 "
                             f"voxels, got {dims}")
    origin, spacing = _origin_spacing("voxelize_mesh", origin, spacing)
    return _voxelize("voxelize_mesh", verts, faces, VOXELIZE_LATTICE, dims, origin, spacing, 0.0,
                     1, dilate, out)


def mesh_occupancy(verts, faces, bound, cascade=None, H: int = 128, dilate=None, out=None):
    """Occupancy prior of a triangle mesh for the marcher's cascade grid: uint8
    [cascade,H,H,H] on the mesh's device, 1 = some face meets the cell's box, 0
    = the mesh does not come near the cell: a shell of cells around the
    surfaces.  ``SemanticNeRFRenderer.set_occupancy_prior`` takes the result.
    ``verts`` / ``faces`` as for ``voxelize_mesh``, in the field's (NGP) frame;
    ``bound`` the renderer's; ``cascade`` None is the renderer's
    ``1 + ceil(log2(bound))``, as in ``tsdf_occupancy``; ``dilate`` (scene
    units, grows every cell's box on all sides) None is one finest cell,
    ``2 * min(1, bound) / H``: a mesh is a surface estimate, and the field's
    surface may sit a cell beside it; ``out`` accumulates as in
    ``voxelize_mesh``.  F = 0 gives an all-zero mask.  Contract of
    ucsa_mesh_voxelize_count / ucsa_mesh_voxelize_fill (include/ucsa_hip.h)."""
    bound = _positive(bound, "mesh_occupancy: bound")
    if cascade is None:
        cascade = 1 + math.ceil(math.log2(bound))
    cascade, H = int(cascade), int(H)
    if not 1 <= cascade <= 31:
        raise _lib.UcsaError(f"mesh_occupancy: cascade must be in 1..31, got {cascade}")
    if not 2 <= H <= 1024:
        raise _lib.UcsaError(f"mesh_occupancy: H must be in 2..1024, got {H}")
    dilate = 2.0 * min(1.0, bound) / H if dilate is None else dilate
    return _voxelize("mesh_occupancy", verts, faces, VOXELIZE_CASCADE, (H, H, H), None, None,
                     bound, cascade, dilate, out)


# ---------------------------------------------------------------------------
# signed distance to a triangle mesh (pseudonormal sign, mesh to TSDF volume)
# ---------------------------------------------------------------------------
def _mesh_i32(verts, faces):
    return _mesh(verts, faces, 0x7FFFFFFF // 3)      # the kernels index 3 F corners


def _normal_runs(items, run_first, n_runs, weight, unit, nf):
    out = torch.zeros((n_runs, 3), dtype=torch.float32, device=unit.device)
    check(lib().ucsa_normal_runs(_ptr(items) if items.numel() else None, _ptr(run_first), n_runs,
                                 int(items.numel()), _ptr(weight), _ptr(unit) if nf else None, nf,
                                 _ptr(out) if n_runs else None, _stream()), "ucsa_normal_runs")
    return out


def mesh_pseudonormals(verts, faces):
    """The normals the sign of ``signed_distance`` / ``mesh_tsdf`` is taken from
    (Baerentzen and Aanaes 2005) -> dict: ``unit_normal`` [F,3] (of
    (B-A)x(C-A); zeros for a degenerate or invalid face), ``corner_angle``
    [F,3] (radians, 0 for an invalid face), ``vertex_normal`` [V,3] (the sum
    over the faces at a vertex of corner angle * unit normal) and
    ``edge_normal`` [F,3,3] (row k of a face: the sum of the unit normals of all
    faces that share its edge corner k -> corner (k+1)%3), all float32 on the
    mesh's device, not normalised: only directions are used.  ``verts`` [V,3]
    float32, ``faces`` [F,3] int32, on the GPU; a face with a corner index
    outside [0,V) or a non-finite corner contributes nothing.  The unit normals
    and the two sums are kernels (ucsa_face_unit_normals, ucsa_normal_runs);
    the corner angles -- atan2(|u x w|, u.w) of the two edges leaving the corner
    -- and the stable sorts that group corners by vertex and half-edges by
    undirected edge are torch on the device.  The sorts are stable, so the
    items of a run ascend in 3f+k and every sum has one order."""
    v, f = _mesh_i32(verts, faces)
    dev = v.device
    nv, nf = int(v.shape[0]), int(f.shape[0])
    unit = torch.zeros((nf, 3), dtype=torch.float32, device=dev)
    check(lib().ucsa_face_unit_normals(_ptr(v) if nv else None, nv, _ptr(f) if nf else None, nf,
                                       _ptr(unit) if nf else None, _stream()),
          "ucsa_face_unit_normals")
    ok = ((f >= 0) & (f < nv)).all(1) if nv else torch.zeros(nf, dtype=torch.bool, device=dev)
    if nv and nf:
        ok &= torch.isfinite(v).all(1)[f.clamp(0, nv - 1).long()].all(1)
    angle = torch.zeros((nf, 3), dtype=torch.float32, device=dev)
    if nv and nf:
        P = v[f.clamp(0, nv - 1).long()]                                # [F,3 corners,3]
        for k in range(3):
            u, w = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            a = torch.atan2(torch.linalg.cross(u, w).norm(dim=1), (u * w).sum(1))
            angle[:, k] = torch.where(ok & torch.isfinite(a), a, torch.zeros_like(a))
    corner = torch.arange(3 * nf, dtype=torch.int32, device=dev)
    valid = ok.repeat_interleave(3)
    items0 = corner[valid]
    flat = f.reshape(-1).long()
    # vertices: the valid corners by vertex index, ties by 3f+k
    vid = flat[valid]
    order = torch.sort(vid, stable=True).indices
    v_items = items0[order].contiguous()
    v_first = torch.searchsorted(vid[order].contiguous(),
                                 torch.arange(nv + 1, dtype=torch.int64, device=dev)
                                 ).to(torch.int32)
    vertex_normal = _normal_runs(v_items, v_first, nv, angle.reshape(-1), unit, nf)
    # edges: the valid half-edges by undirected edge, ties by 3f+k
    nxt = f[:, [1, 2, 0]].reshape(-1).long()
    a, b = flat[valid], nxt[valid]
    key = torch.minimum(a, b) * max(nv, 1) + torch.maximum(a, b)
    order = torch.sort(key, stable=True).indices
    e_items = items0[order].contiguous()
    skey = key[order]
    n_half = int(skey.numel())
    head = torch.ones(n_half, dtype=torch.bool, device=dev)
    if n_half > 1:
        head[1:] = skey[1:] != skey[:-1]
    starts = torch.nonzero(head).reshape(-1)
    n_edges = int(starts.numel())
    e_first = torch.empty(n_edges + 1, dtype=torch.int32, device=dev)
    e_first[:n_edges] = starts
    e_first[n_edges] = n_half
    sums = _normal_runs(e_items, e_first, n_edges, None, unit, nf)
    edge_normal = torch.zeros((3 * nf, 3), dtype=torch.float32, device=dev)
    if n_half:
        edge_normal[e_items.long()] = sums[torch.cumsum(head, 0) - 1]
    return {"unit_normal": unit, "corner_angle": angle, "vertex_normal": vertex_normal,
            "edge_normal": edge_normal.view(nf, 3, 3)}


def _normals_args(normals, nv, nf, dev):
    try:
        un, vn, en = normals["unit_normal"], normals["vertex_normal"], normals["edge_normal"]
    except (TypeError, KeyError):
        raise _lib.UcsaError("normals must be the dict of ops.mesh_pseudonormals")
    for t, shape, name in ((un, (nf, 3), "unit_normal"), (vn, (nv, 3), "vertex_normal"),
                           (en, (nf, 3, 3), "edge_normal")):
        _gpu(t, f"normals: {name} (a different mesh?)", torch.float32, shape, device=dev,
             fixed=True)
    return (_ptr(un) if nf else None, _ptr(vn) if nv else None, _ptr(en) if nf else None)


def signed_distance(grid, normals, verts, faces, queries, max_dist: float,
                    sort_queries: bool = True):
    """For each of ``queries`` [Q,3] the signed distance to the mesh ``verts`` /
    ``faces`` within ``max_dist`` -> (``sdf`` float32 [Q], ``face``, ``dist2``,
    ``bary``, ``feature`` int32 [Q]): ``nearest_triangle`` (``grid`` is
    ``triangle_grid``'s dict of the same mesh; face, dist2 and bary are its
    outputs) followed by the sign.  ``abs(sdf)`` is ``sqrt(dist2)``; the sign is
    that of the angle-weighted pseudonormal (``normals``:
    ``mesh_pseudonormals``'s dict) of the feature the closest point lies on:
    ``feature`` 0 the face's interior, 1..3 its edges AB, BC, CA, 4..6 its
    corners A, B, C.  Positive is the side (B-A)x(C-A) points to: outside a
    mesh whose faces are counter-clockwise seen from outside.  No face within
    ``max_dist``: +inf and feature -1; a query on the surface: +0.  The sign is
    right wherever the mesh is a consistently oriented surface near the query;
    it is not a winding number and does not repair a badly oriented mesh.
    Contract of ucsa_mesh_sign (include/ucsa_hip.h)."""
    v, f = _mesh_i32(verts, faces)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    try:
        grid_faces = int(grid["n_faces"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    if grid_faces != nf:
        raise _lib.UcsaError(f"grid was built over {grid_faces} faces, the mesh has {nf}")
    un, vn, en = _normals_args(normals, nv, nf, v.device)
    face, dist2, bary = nearest_triangle(grid, queries, max_dist, sort_queries)
    q = _points3(queries, "queries")
    if q.device != v.device:
        raise _lib.UcsaError(f"the mesh is on {v.device}, the queries on {q.device}")
    nq = int(q.shape[0])
    sdf = torch.empty(nq, dtype=torch.float32, device=q.device)
    feature = torch.empty(nq, dtype=torch.int32, device=q.device)
    check(lib().ucsa_mesh_sign(_ptr(v) if nv else None, nv, _ptr(f) if nf else None, nf, un, vn,
                               en, _ptr(q), nq, _ptr(face), _ptr(sdf), _ptr(feature), _stream()),
          "ucsa_mesh_sign")
    return sdf, face, dist2, bary, feature


def mesh_tsdf(volume, verts, faces, trunc: float, weight: float = 1.0, grid=None, normals=None):
    """Write the truncated signed distance to a mesh into ``volume``
    (``tsdf_volume``), in place; returns ``volume``.  Every voxel within
    ``trunc`` (scene units, inclusive) of the surface gets
    ``tsdf = clamp(sdf / trunc, -1, 1)`` and ``weight = weight``; every other
    voxel keeps what it held, so a fresh volume stays free and unobserved
    outside the band, as after ``integrate_tsdf``, and ``raycast_tsdf``,
    ``marching_cubes(valid=)``, ``tsdf_occupancy`` and ``voxel_components`` take
    the result.  The band is overwritten: the mesh is not averaged with what
    the volume held there, and ``rgb`` is not touched.  The sign is
    ``signed_distance``'s (positive on the side (B-A)x(C-A) points to, which is
    free space for a mesh that is counter-clockwise seen from outside).
    ``grid`` / ``normals`` are ``triangle_grid``'s and ``mesh_pseudonormals``'s
    dicts of the mesh, built here when not given.  One launch
    (ucsa_mesh_tsdf, include/ucsa_hip.h): the search runs from the lattice
    points themselves, byte for byte ``signed_distance`` on the materialised
    lattice."""
    (nx, ny, nz), dev = volume_lattice(volume)
    v, f = _mesh_i32(verts, faces)
    if v.device != dev:
        raise _lib.UcsaError(f"the volume is on {dev}, the mesh on {v.device}")
    nv, nf = int(v.shape[0]), int(f.shape[0])
    trunc = _positive(trunc, "mesh_tsdf: trunc")
    weight = float(weight)
    if math.isnan(weight):
        raise _lib.UcsaError("mesh_tsdf: weight must not be NaN")
    origin = [float(x) for x in volume["origin"]]
    spacing = [float(x) for x in volume["spacing"]]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("mesh_tsdf: origin and spacing have 3 entries each")
    if grid is None:
        grid = triangle_grid(v, f)
    if normals is None:
        normals = mesh_pseudonormals(v, f)
    try:
        rec, offsets, n = grid["records"], grid["offsets"], int(grid["n_pairs"])
        g_origin, cell, dims, grid_faces = grid["origin"], float(grid["cell"]), grid["dims"], \
            int(grid["n_faces"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    _gpu(rec, "grid: records", torch.float32, (n, 12), device=dev, fixed=True)
    _gpu(offsets, "grid: offsets", torch.int32, numel=ncells + 1, device=dev, fixed=True)
    if grid_faces != nf:
        raise _lib.UcsaError(f"grid was built over {grid_faces} faces, the mesh has {nf}")
    un, vn, en = _normals_args(normals, nv, nf, dev)
    check(lib().ucsa_mesh_tsdf(
        _ptr(rec) if n else None, _ptr(offsets) if n else None, n, fvec(g_origin), cell,
        (C.c_uint32 * 3)(*[int(d) for d in dims]), _ptr(v) if nv else None, nv,
        _ptr(f) if nf else None, nf, un, vn, en, _ptr(volume["tsdf"]), _ptr(volume["weight"]),
        nx, ny, nz, fvec(origin), fvec(spacing), trunc, weight, _stream()), "ucsa_mesh_tsdf")
    return volume
