"""Registration of points to a triangle mesh: the fused step of ICP over the
grid of ``ops.triangle_grid``.  Reached as ``ops.register.icp_sums``.  The same
step against a TSDF volume, without a mesh: ``ops.register.tsdf_sums``; and
against a pair of vertex and normal maps, by projection:
``ops.register.projective_sums``.  Many rigid hypotheses scored against a TSDF
volume in one call, for a global search: ``ops.register.tsdf_scores``; the TSDF
step for K hypotheses in one call: ``ops.register.tsdf_sums_batch``."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import _gpu, _mesh, _origin_spacing, _points3, _positive, _ptr, _stream, volume_lattice

ICP_SUMS = 29
MODES = {"plane": 0, "point": 1}
_EDGE, _GRAZING = 4, 8  # ops.depth's mask bits (UCSA_DEPTH_EDGE, UCSA_DEPTH_GRAZING)
TSDF_SCORE_TILE = 16    # transforms per work-group of k_tsdf_score (UCSA_TSDF_SCORE_TILE)
TSDF_SCORE_MAX_POINTS = 1 << 23
TSDF_SUMS_BATCH_TILE = 8     # transforms per work-group of k_tsdf_icp_sums_batch
TSDF_SUMS_BATCH_MAX = 1024   # transforms per call (UCSA_TSDF_ICP_BATCH_MAX)


def workspace_rows(n: int) -> int:
    """the rows of 29 doubles ``ucsa_icp_sums`` keeps between its reduce stages"""
    rows, c = 0, max(1, -(-int(n) // 256))
    while c > 1:
        rows += c
        c = -(-c // 256)
    return rows


def _transform12(transform):
    """a 3x4 or 4x4 array-like on the host -> the 12 floats of its first three rows"""
    try:
        t = torch.as_tensor(transform, dtype=torch.float64, device="cpu")
    except (TypeError, ValueError, RuntimeError):
        raise _lib.UcsaError(f"transform must be a 3x4 or 4x4 array on the host, got "
                             f"{type(transform).__name__}")
    if tuple(t.shape) not in ((3, 4), (4, 4)):
        raise _lib.UcsaError(f"transform must be 3x4 or 4x4, got {tuple(t.shape)}")
    return fvec(t[:3].to(torch.float32).reshape(-1).tolist())


def _volume_points(volume, points, max_rows: int, limit: str):
    """the checked lattice of a TSDF ``volume`` and ``points`` [N,3] on its device, at most
    ``max_rows`` (named ``limit``) -> ((nx, ny, nz), device, origin, spacing, points, N)"""
    (nx, ny, nz), dev = volume_lattice(volume)
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7FFFFFFF:
        raise _lib.UcsaError(f"volume: dims must be >= 2 each with at most 2^31-1 points, got "
                             f"{(nx, ny, nz)}")
    origin, spacing = _origin_spacing("volume", volume["origin"], volume["spacing"])
    pts = _gpu(points, "points", torch.float32, (None, 3), device=dev)
    n = int(pts.shape[0])
    if n > max_rows:
        raise _lib.UcsaError(f"points must have at most {limit} rows")
    return (nx, ny, nz), dev, origin, spacing, pts, n


def _device_transforms(transforms, dev, too_many):
    """float32 [K,3,4] or [K,4,4] on ``dev`` -> (the contiguous rows [K,3,4], K);
    ``too_many(K)`` is the error's message for a K beyond the caller's limit, else None"""
    T = _gpu(transforms, "transforms", torch.float32, (None, None, 4), device=dev)
    if T.shape[1] not in (3, 4):
        raise _lib.UcsaError(f"transforms must be [K,3,4] or [K,4,4], got {tuple(T.shape)}")
    T = T[:, :3].contiguous()
    K = int(T.shape[0])
    if too_many(K):
        raise _lib.UcsaError(too_many(K))
    return T, K


def _sample_gates(min_weight, max_tsdf, closed: bool):
    """``min_weight`` > 0 and ``max_tsdf`` in (0, 1] -- in (0, 1) when not ``closed`` -- as floats"""
    min_weight = float(min_weight)
    if not min_weight > 0:
        raise _lib.UcsaError(f"min_weight must be > 0, got {min_weight!r}")
    max_tsdf = float(max_tsdf)
    if not (0 < max_tsdf <= 1 if closed else 0 < max_tsdf < 1):
        raise _lib.UcsaError(f"max_tsdf must be in (0, 1{']' if closed else ')'}, got "
                             f"{max_tsdf!r}")
    return min_weight, max_tsdf


def _sums_buffers(n: int, dev, K=None):
    """-> (the workspace or None when one stage suffices, its size in doubles, ``sums``
    uninitialised: [29], or [K,29] for K transforms)"""
    ws_doubles = (1 if K is None else K) * ICP_SUMS * workspace_rows(n)
    ws = torch.empty(ws_doubles, dtype=torch.float64, device=dev) if ws_doubles else None
    shape = ICP_SUMS if K is None else (K, ICP_SUMS)
    return ws, ws_doubles, torch.empty(shape, dtype=torch.float64, device=dev)


def face_unit_normals(verts, faces):
    """The unit normals of a mesh's faces -> float32 [F,3] on its device: the
    ``unit_normal`` of ``ops.mesh_pseudonormals`` without the vertex and edge
    sums (ucsa_face_unit_normals: zeros for a degenerate or invalid face)."""
    v, f = _mesh(verts, faces)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    unit = torch.zeros((nf, 3), dtype=torch.float32, device=v.device)
    check(lib().ucsa_face_unit_normals(_ptr(v) if nv else None, nv, _ptr(f) if nf else None, nf,
                                       _ptr(unit) if nf else None, _stream()),
          "ucsa_face_unit_normals")
    return unit


def cell_order(grid, points, transform):
    """The order that sorts ``points`` [N,3] by the cell of ``grid`` their moved
    position q = R p + t falls in (ties by index) -> int32 [N] on the device.
    The move is elementwise torch and the keys are ucsa_point_cell_keys, as for
    the queries of ``nearest_triangle``: it orders lanes and changes no result
    but, through the summation tree of ``icp_sums``, last bits."""
    pts = _points3(points, "points")
    n = int(pts.shape[0])
    T = torch.as_tensor(transform, dtype=torch.float64)[:3].to(torch.float32).to(pts.device)
    q = pts[:, 0:1] * T[:, 0] + pts[:, 1:2] * T[:, 1] + pts[:, 2:3] * T[:, 2] + T[:, 3]
    q = q.contiguous()
    try:
        origin, cell, dims = grid["origin"], float(grid["cell"]), grid["dims"]
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    keys = torch.empty(n, dtype=torch.int32, device=pts.device)
    if n:
        check(lib().ucsa_point_cell_keys(_ptr(q), n, fvec(origin), cell,
                                         (C.c_uint32 * 3)(*[int(d) for d in dims]), 0, _ptr(keys),
                                         _stream()), "ucsa_point_cell_keys")
    return torch.sort(keys, stable=True).indices.to(torch.int32)


def icp_sums(grid, verts, faces, unit_normal, points, transform, max_dist: float,
             mode: str = "plane", return_matches: bool = False):
    """The normal equations of one ICP step of ``points`` [N,3] (float32 on the
    GPU) against the mesh ``verts`` / ``faces`` -> ``sums`` float64 [29] on the
    device, or (``sums``, ``face`` int32 [N], ``dist2`` float32 [N]) with
    ``return_matches``.  One call moves every point by ``transform`` (a 3x4 or
    4x4 array-like on the host, converted to float32: q = R p + t), finds q's
    closest point on the mesh within ``max_dist`` -- ``nearest_triangle``'s
    search, whose ``face`` and ``dist2`` for q the matches are -- and sums over
    the matched points, in float64 and in a fixed tree, the 21 entries of the
    upper triangle of J^T J (row-major), the 6 of J^T r, r^2 and 1 (the count).
    ``mode`` "plane": one row per point, r the distance to the closest point
    along the face's unit normal n, J = (q x n, n); "point": three rows, n the
    axes.  ``grid`` is ``triangle_grid``'s dict of the same mesh and
    ``unit_normal`` [F,3] float32 the ``unit_normal`` of ``mesh_pseudonormals``
    (ucsa_face_unit_normals).  The points are taken in the order given: the sums
    are defined on it and no sort happens here.  ``utils.registration`` turns
    the sums into a step.  Contract of ucsa_icp_sums (include/ucsa_hip.h)."""
    v, f = _mesh(verts, faces)
    dev = v.device
    nv, nf = int(v.shape[0]), int(f.shape[0])
    pts = _points3(points, "points")
    if pts.device != dev:
        raise _lib.UcsaError(f"the mesh is on {dev}, the points on {pts.device}")
    n = int(pts.shape[0])
    un = _gpu(unit_normal, "unit_normal (a different mesh?)", torch.float32, (nf, 3), device=dev)
    try:
        rec, offsets, P = grid["records"], grid["offsets"], int(grid["n_pairs"])
        origin, cell, dims, grid_faces = grid["origin"], float(grid["cell"]), grid["dims"], \
            int(grid["n_faces"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    _gpu(rec, "grid: records", torch.float32, (P, 12), device=dev, fixed=True)
    _gpu(offsets, "grid: offsets", torch.int32, numel=ncells + 1, device=dev, fixed=True)
    if grid_faces != nf:
        raise _lib.UcsaError(f"grid was built over {grid_faces} faces, the mesh has {nf}")
    max_dist = _positive(max_dist, "max_dist")
    if mode not in MODES:
        raise _lib.UcsaError(f"mode must be 'plane' or 'point', got {mode!r}")
    t12 = _transform12(transform)
    ws, ws_doubles, sums = _sums_buffers(n, dev)
    face = torch.empty(n, dtype=torch.int32, device=dev) if return_matches else None
    dist2 = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    check(lib().ucsa_icp_sums(
        _ptr(rec) if P else None, _ptr(offsets) if P else None, P, fvec(origin), cell,
        (C.c_uint32 * 3)(*[int(d) for d in dims]), _ptr(v) if nv else None, nv,
        _ptr(f) if nf else None, nf, _ptr(un) if nf else None, _ptr(pts) if n else None, n, t12,
        max_dist, MODES[mode], _ptr(ws), ws_doubles, _ptr(sums), _ptr(face), _ptr(dist2),
        _stream()), "ucsa_icp_sums")
    return (sums, face, dist2) if return_matches else sums


def _tsdf_step_args(volume, points, transform, trunc, min_weight, max_tsdf):
    """the checked arguments ``tsdf_sums`` and ``tsdf_sums_weighted`` share"""
    (nx, ny, nz), dev, origin, spacing, pts, n = \
        _volume_points(volume, points, 0x7FFFFFFF, "2^31-1")
    t12 = _transform12(transform)
    trunc = _positive(trunc, "trunc")
    min_weight, max_tsdf = _sample_gates(min_weight, max_tsdf, True)
    return (nx, ny, nz), dev, origin, spacing, pts, n, t12, trunc, min_weight, max_tsdf


def tsdf_sums(volume, points, transform, trunc: float, min_weight: float = 1.0,
              max_tsdf: float = 1.0, return_matches: bool = False):
    """The normal equations of one point-to-plane ICP step of ``points`` [N,3]
    (float32 on the GPU) against the TSDF ``volume`` (``ops.tsdf_volume``'s dict,
    as ``ops.integrate_tsdf`` leaves it) -> ``sums`` float64 [29] on the device,
    or (``sums``, ``value`` float32 [N], ``matched`` uint8 [N]) with
    ``return_matches``.  One call moves every point by ``transform`` (a 3x4 or
    4x4 array-like on the host, converted to float32: q = R p + t), samples the
    volume at q -- the trilinear value F and the gradient that
    ``ops.raycast_tsdf`` writes as its normal n, from the cell's sixteen loads --
    and sums over the matched points r = -(F * trunc) and J = (q x n, n) as
    ``icp_sums`` does in mode "plane": the same 29 float64 numbers in the same
    tree, so ``utils.registration.solve_step`` and ``compose`` take them
    unchanged.  A point matches when it lies inside the lattice (it is not
    clamped into it), all eight corners of its cell have weight >=
    ``min_weight``, the gradient is not zero and |F| <= ``max_tsdf`` (in units
    of ``trunc``, at most 1: the coarse-to-fine gate).  ``trunc`` is the
    truncation distance the volume was integrated with.  ``value`` is F where
    the cell is observed and NaN elsewhere.  Contract of ucsa_tsdf_icp_sums
    (include/ucsa_hip.h)."""
    (nx, ny, nz), dev, origin, spacing, pts, n, t12, trunc, min_weight, max_tsdf = \
        _tsdf_step_args(volume, points, transform, trunc, min_weight, max_tsdf)
    ws, ws_doubles, sums = _sums_buffers(n, dev)
    value = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    matched = torch.empty(n, dtype=torch.uint8, device=dev) if return_matches else None
    check(lib().ucsa_tsdf_icp_sums(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        _ptr(pts) if n else None, n, t12, trunc, min_weight, max_tsdf, _ptr(ws), ws_doubles,
        _ptr(sums), _ptr(value), _ptr(matched), _stream()), "ucsa_tsdf_icp_sums")
    return (sums, value, matched) if return_matches else sums


def tsdf_sums_batch(volume, points, transforms, trunc: float, min_weight: float = 1.0,
                    max_tsdf: float = 1.0):
    """``tsdf_sums`` for K rigid hypotheses of the same ``points`` [N,3] (float32
    on the GPU) against the same TSDF ``volume`` in one call -> float64 [K,29] on
    the device.  ``transforms`` is float32 [K,3,4] or [K,4,4] on the volume's
    device, as for ``tsdf_scores`` (the first three rows are taken: q = R p + t).
    Row k holds, as int64 words, what ``tsdf_sums(volume, points, transforms[k],
    trunc, min_weight, max_tsdf)`` returns: the same float32 expressions and the
    same tree per row, whatever K and wherever the row stands in the batch.
    There are no per-point outputs.  At most 2^23 points and
    ``TSDF_SUMS_BATCH_MAX`` transforms; K = 0 gives an empty result.
    ``utils.registration.register_points_tsdf_batch`` iterates K loops in lock
    step on it.  Contract of ucsa_tsdf_icp_sums_batch (include/ucsa_hip.h)."""
    (nx, ny, nz), dev, origin, spacing, pts, n = \
        _volume_points(volume, points, TSDF_SCORE_MAX_POINTS, "2^23")
    T, K = _device_transforms(transforms, dev, lambda K: K > TSDF_SUMS_BATCH_MAX and (
        f"transforms must have at most {TSDF_SUMS_BATCH_MAX} rows, got {K}"))
    trunc = _positive(trunc, "trunc")
    min_weight, max_tsdf = _sample_gates(min_weight, max_tsdf, True)
    ws, ws_doubles, sums = _sums_buffers(n, dev, K)
    check(lib().ucsa_tsdf_icp_sums_batch(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        _ptr(pts) if n else None, n, _ptr(T) if K else None, K, trunc, min_weight, max_tsdf,
        _ptr(ws), ws_doubles, _ptr(sums) if K else None, _stream()), "ucsa_tsdf_icp_sums_batch")
    return sums


def tsdf_scores(volume, points, transforms, min_weight: float = 1.0, max_tsdf: float = 0.75):
    """The scores of K rigid hypotheses of ``points`` [N,3] (float32 on the GPU)
    against the TSDF ``volume`` (``ops.tsdf_volume``'s dict) -> int64 [K,4] on the
    device, in one call.  ``transforms`` is float32 [K,3,4] or [K,4,4] on the
    volume's device (the first three rows are taken: q = R p + t); it stays on
    the device because there can be millions.  Per transform the row is
    (inliers, free, sum e, sum e^2) over the points: a moved point is sampled
    as ``tsdf_sums`` samples it (inside the lattice, all eight corners of its
    cell with weight >= ``min_weight``, the trilinear value F); it is an inlier
    when |F| <= ``max_tsdf``, it lies in free space -- where the volume saw
    nothing -- when F > ``max_tsdf``, and e = rint(|F| * 2^20) of an inlier.
    All four are exact integers: the bytes depend neither on the order of the
    points nor on anything else that varies between runs.  ``max_tsdf`` lies in
    (0, 1): at 1 free space would count as inlier.  At most 2^23 points.
    ``utils.registration.global_register_points_tsdf`` ranks hypotheses by
    inliers - free, then sum e^2.  Contract of ucsa_tsdf_score_transforms
    (include/ucsa_hip.h)."""
    (nx, ny, nz), dev, origin, spacing, pts, n = \
        _volume_points(volume, points, TSDF_SCORE_MAX_POINTS, "2^23")
    T, K = _device_transforms(transforms, dev, lambda K: K > 0x7FFFFFFF and (
        "transforms must have at most 2^31-1 rows"))
    min_weight, max_tsdf = _sample_gates(min_weight, max_tsdf, False)
    scores = torch.empty((K, 4), dtype=torch.int64, device=dev)
    check(lib().ucsa_tsdf_score_transforms(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        _ptr(pts) if n else None, n, _ptr(T) if K else None, K, min_weight, max_tsdf,
        _ptr(scores) if K else None, _stream()), "ucsa_tsdf_score_transforms")
    return scores


def _projective_step_args(points, normals, target_points, target_normals, target_mask,
                          intrinsics, transform, max_dist, min_cos, reject):
    """the checked arguments ``projective_sums`` and ``projective_sums_weighted`` share"""
    pts = _points3(points, "points")
    dev = pts.device
    n = int(pts.shape[0])
    nrm = None if normals is None else _gpu(normals, "normals", torch.float32, (n, 3), device=dev)
    tp = _gpu(target_points, "target_points", torch.float32, (None, None, 3), device=dev)
    H, W = int(tp.shape[0]), int(tp.shape[1])
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise _lib.UcsaError(f"target_points must be [H,W,3] with 1 <= H, W <= 16384, got "
                             f"{tuple(tp.shape)}")
    tn = _gpu(target_normals, "target_normals", torch.float32, (H, W, 3), device=dev)
    tm = _gpu(target_mask, "target_mask", torch.uint8, (H, W), device=dev)
    try:
        fx, fy, cx, cy = [float(v) for v in intrinsics]
    except (TypeError, ValueError):
        raise _lib.UcsaError("intrinsics must be (fx, fy, cx, cy)")
    if not (fx > 0 and fy > 0 and all(math.isfinite(v) for v in (fx, fy, cx, cy))):
        raise _lib.UcsaError(f"intrinsics must have fx, fy > 0 and be finite, got "
                             f"{(fx, fy, cx, cy)}")
    t12 = _transform12(transform)
    max_dist = _positive(max_dist, "max_dist")
    min_cos = float(min_cos)
    if not -1.0 <= min_cos <= 1.0:
        raise _lib.UcsaError(f"min_cos must be in [-1, 1], got {min_cos!r}")
    if isinstance(reject, bool) or not isinstance(reject, int) or reject & ~(_EDGE | _GRAZING):
        raise _lib.UcsaError(f"reject must be a set of EDGE (4) | GRAZING (8), got {reject!r}")
    return dev, pts, n, nrm, tp, tn, tm, H, W, (fx, fy, cx, cy), t12, max_dist, min_cos


def projective_sums(points, normals, target_points, target_normals, target_mask, intrinsics,
                    transform, max_dist: float, min_cos: float = 0.0,
                    reject: int = _EDGE | _GRAZING, return_matches: bool = False):
    """The normal equations of one projective point-to-plane ICP step of
    ``points`` [N,3] (float32 on the GPU) against a pair of maps -> ``sums``
    float64 [29] on the device, or (``sums``, ``pixel`` int32 [N], ``residual``
    float32 [N]) with ``return_matches``.  The maps are ``target_points`` and
    ``target_normals`` [H,W,3] float32 in the target camera's frame and
    ``target_mask`` [H,W] uint8 (``ops.depth.depth_normals``' outputs for one
    frame, or a model ray-cast dressed the same way); ``intrinsics`` (fx, fy,
    cx, cy) is the target camera.  One call moves every point by ``transform``
    (a 3x4 or 4x4 array-like on the host, converted to float32: source frame ->
    target camera frame, q = R p + t), projects q into the target image with
    ``ops.integrate_tsdf``'s expression and gathers the pixel it falls in: no
    search.  The pair matches when the pixel has a normal (mask bit 2), carries
    no bit of ``reject`` (a set of EDGE (4) | GRAZING (8)), its six floats are
    finite, the target point c lies within ``max_dist`` of q and -- with source
    ``normals`` [N,3]; None: no such gate -- the rotated source normal and the
    target normal nt have a cosine >= ``min_cos``.  Over the matched points
    r = nt . (c - q) and J = (q x nt, nt) are summed as ``icp_sums`` does in mode
    "plane": the same 29 float64 numbers in the same tree, so
    ``utils.registration.solve_step`` and ``compose`` take them unchanged.
    ``pixel`` is the matched pixel's row-major index or -1, ``residual`` r or
    NaN.  Contract of ucsa_projective_icp_sums (include/ucsa_hip.h)."""
    dev, pts, n, nrm, tp, tn, tm, H, W, (fx, fy, cx, cy), t12, max_dist, min_cos = \
        _projective_step_args(points, normals, target_points, target_normals, target_mask,
                              intrinsics, transform, max_dist, min_cos, reject)
    ws, ws_doubles, sums = _sums_buffers(n, dev)
    pixel = torch.empty(n, dtype=torch.int32, device=dev) if return_matches else None
    residual = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    check(lib().ucsa_projective_icp_sums(
        _ptr(pts) if n else None, _ptr(nrm) if n else None, n, _ptr(tp), _ptr(tn), _ptr(tm), H, W,
        reject, fx, fy, cx, cy, t12, max_dist, min_cos, _ptr(ws), ws_doubles, _ptr(sums),
        _ptr(pixel), _ptr(residual), _stream()), "ucsa_projective_icp_sums")
    return (sums, pixel, residual) if return_matches else sums


ROBUST = {"none": 0, "huber": 1, "tukey": 2}  # UCSA_ROBUST_NONE / HUBER / TUKEY


def _robust_args(point_weight, robust, robust_scale, n, dev):
    """the checked weight arguments of the two weighted steps -> (weights or None,
    kind, scale)"""
    if robust not in ROBUST:
        raise _lib.UcsaError(f"robust must be 'none', 'huber' or 'tukey', got {robust!r}")
    scale = 1.0
    if ROBUST[robust]:
        if robust_scale is None:
            raise _lib.UcsaError(f"robust={robust!r} needs a robust_scale")
        scale = _positive(robust_scale, "robust_scale")
    pw = None if point_weight is None else \
        _gpu(point_weight, "point_weight", torch.float32, (n,), device=dev)
    return pw, ROBUST[robust], scale


def projective_sums_weighted(points, normals, target_points, target_normals, target_mask,
                             intrinsics, transform, max_dist: float, min_cos: float = 0.0,
                             reject: int = _EDGE | _GRAZING, point_weight=None,
                             robust: str = "none", robust_scale=None,
                             return_matches: bool = False):
    """``projective_sums`` with a weight per row: one step of iteratively
    reweighted least squares -> ``sums`` float64 [29] on the device, or
    (``sums``, ``pixel``, ``residual``, ``weight`` float32 [N]) with
    ``return_matches``.  Association, gates and the row (J, r) are
    ``projective_sums``'.  Then, in float32, w = p * rho(|r|): p is
    ``point_weight`` [N] (float32 on the GPU; None: 1; a p that is not finite
    and > 0 takes the point out, ``ops.integrate_tsdf_weighted``'s rule for a
    pixel) and rho the kernel ``robust``: "none" 1; "huber" 1 for |r| <= k, else
    k / |r|; "tukey" (1 - (|r| / c)^2)^2 for |r| < c, else 0, with k or c =
    ``robust_scale`` in the residual's units.  A row counts when it matched and
    w > 0; it enters scaled by sqrt(w), so the sums are sum w J^T J, sum w J^T r,
    sum w r^2 and the number of rows that count, in ``projective_sums``' layout
    and tree: ``utils.registration.solve_step`` and ``compose`` take them
    unchanged.  ``weight`` is w for a row that counts and 0 otherwise;
    ``pixel`` and ``residual`` (the unscaled r) report the geometric match.
    With "none" and no ``point_weight`` the sums equal ``projective_sums``' as
    int64 words.  Contract of ucsa_projective_icp_sums_weighted
    (include/ucsa_hip.h)."""
    dev, pts, n, nrm, tp, tn, tm, H, W, (fx, fy, cx, cy), t12, max_dist, min_cos = \
        _projective_step_args(points, normals, target_points, target_normals, target_mask,
                              intrinsics, transform, max_dist, min_cos, reject)
    pw, kind, scale = _robust_args(point_weight, robust, robust_scale, n, dev)
    ws, ws_doubles, sums = _sums_buffers(n, dev)
    pixel = torch.empty(n, dtype=torch.int32, device=dev) if return_matches else None
    residual = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    weight = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    check(lib().ucsa_projective_icp_sums_weighted(
        _ptr(pts) if n else None, _ptr(nrm) if n else None, n, _ptr(tp), _ptr(tn), _ptr(tm), H, W,
        reject, fx, fy, cx, cy, t12, max_dist, min_cos, _ptr(pw) if n else None, kind, scale,
        _ptr(ws), ws_doubles, _ptr(sums), _ptr(pixel), _ptr(residual), _ptr(weight), _stream()),
        "ucsa_projective_icp_sums_weighted")
    return (sums, pixel, residual, weight) if return_matches else sums


def tsdf_sums_weighted(volume, points, transform, trunc: float, min_weight: float = 1.0,
                       max_tsdf: float = 1.0, point_weight=None, robust: str = "none",
                       robust_scale=None, return_matches: bool = False):
    """``tsdf_sums`` with a weight per row, as ``projective_sums_weighted`` is to
    ``projective_sums`` -> ``sums`` float64 [29] on the device, or (``sums``,
    ``value``, ``matched``, ``weight`` float32 [N]) with ``return_matches``.  The
    sample, the gates and the row (J, r = -(F * trunc)) are ``tsdf_sums``'; the
    weight w = p * rho(|r|), the rows that count, the scaling by sqrt(w) and the
    meaning of the 29 sums are ``projective_sums_weighted``'s, ``robust_scale``
    in scene units like r.  ``value`` and ``matched`` report the geometric
    match.  With "none" and no ``point_weight`` the sums equal ``tsdf_sums``' as
    int64 words.  Contract of ucsa_tsdf_icp_sums_weighted (include/ucsa_hip.h)."""
    (nx, ny, nz), dev, origin, spacing, pts, n, t12, trunc, min_weight, max_tsdf = \
        _tsdf_step_args(volume, points, transform, trunc, min_weight, max_tsdf)
    pw, kind, scale = _robust_args(point_weight, robust, robust_scale, n, dev)
    ws, ws_doubles, sums = _sums_buffers(n, dev)
    value = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    matched = torch.empty(n, dtype=torch.uint8, device=dev) if return_matches else None
    weight = torch.empty(n, dtype=torch.float32, device=dev) if return_matches else None
    check(lib().ucsa_tsdf_icp_sums_weighted(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        _ptr(pts) if n else None, n, t12, trunc, min_weight, max_tsdf, _ptr(pw) if n else None,
        kind, scale, _ptr(ws), ws_doubles, _ptr(sums), _ptr(value), _ptr(matched), _ptr(weight),
        _stream()), "ucsa_tsdf_icp_sums_weighted")
    return (sums, value, matched, weight) if return_matches else sums
