"""Rigid registration of points to a triangle mesh: iterated closest point over
``ops.register.icp_sums``.

One iteration is one fused launch on the device (transform, closest point on the
mesh, the Gauss-Newton normal equations as 29 float64 sums in a fixed tree), one
read of those 29 doubles and a 6 x 6 solve on the host.  The host half
(``normal_equations``, ``solve_step``, ``compose``) is plain numpy float64 and
needs no GPU; ``register_points`` and what sits on it do.

The step: with q the moved point, p the vector from q to its closest point and
n the row's normal (the face's unit normal in mode "plane", the three axes in
mode "point"), r = n . p and J = (q x n, n) linearise the move
q <- q + omega x q + upsilon, and the step minimises sum (r - J . xi)^2 over
xi = (omega, upsilon): (sum J^T J) xi = sum J^T r.

Both uses go through ``register_points``: mesh to mesh (``register_meshes``: align
a fused or exported mesh to the ground truth before it is scored) and depth
frame to mesh (``refine_pose``: the points are back-projected in the camera frame
and the initial transform is the camera pose, so the result is a refined pose).

``register_points_tsdf`` / ``refine_pose_tsdf`` run the same loop against a TSDF
volume instead of a mesh (``ops.register.tsdf_sums``: the residual is the
volume's signed distance at the moved point, the normal its gradient), for a
pose already within the truncation distance of the answer: frame-to-model
tracking while a scene is fused (``utils.tsdf_fusion.track_depth_views``).

``register_frames`` / ``odometry`` / ``refine_pose_projective`` are KinectFusion's
own tracker (``ops.register.projective_sums``): a frame's vertex and normal maps
on a depth pyramid (``frame_maps``) against a second pair of maps -- the frame
before it, or the model ray-cast from the last pose -- matched by projection, a
gather in place of a search, with a distance and a normal-compatibility gate.

``global_register_points_tsdf`` / ``global_register_meshes`` find the coarse
alignment those loops start from: hypotheses over a rotation set scored against
a TSDF volume in one call (``ops.register.tsdf_scores``), the best refined --
one after another, or with ``lockstep`` all together
(``register_points_tsdf_batch`` over ``ops.register.tsdf_sums_batch``).

The two frame trackers (``register_frames`` and ``register_points_tsdf`` with what
sits on them) take ``robust`` / ``robust_scale`` / ``point_weight`` and, for the
frames, ``view_weights``: iteratively reweighted least squares over
``ops.register.projective_sums_weighted`` / ``tsdf_sums_weighted``, for frames
that show something their target does not.  Off by default; for the tracking
regime only (a redescending kernel narrows the basin).

Not here: scale, rejection of matches on open boundaries, normal compatibility
gates in the mesh and TSDF routes, robust kernels in the mesh route and the
lock-step batch, scales estimated from the data: the local loops must start
within ``max_dist`` (or ``trunc``) and a few degrees of the answer."""
from __future__ import annotations

import math

import numpy as np

SUMS = 29
_PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


# ---------------------------------------------------------------------------
# the host half: numpy float64, no GPU
# ---------------------------------------------------------------------------
def normal_equations(sums):
    """``icp_sums``' 29 doubles -> (``A`` [6,6] = sum J^T J, ``b`` [6] = sum J^T r,
    ``sse`` = sum r^2, ``count`` = the rows summed: the matched points in mode
    "plane", three times as many in mode "point")."""
    s = np.asarray(sums, np.float64).reshape(-1)
    if s.size != SUMS:
        raise ValueError(f"sums must have {SUMS} entries, got {s.size}")
    A = np.zeros((6, 6), np.float64)
    for k, (a, b) in enumerate(_PAIRS):
        A[a, b] = A[b, a] = s[k]
    return A, s[21:27].copy(), float(s[27]), float(s[28])


def solve_step(sums, rcond: float = 1e-8):
    """The Gauss-Newton step of one iteration -> (``xi`` [6] = (omega, upsilon),
    ``rank``).  The rule: the rotation columns are divided by a characteristic
    length L = sqrt(trace(A[:3,:3]) / trace(A[3:,3:])) -- the rms lever arm of the
    rows, 1 if either trace is not positive -- so that rotation and translation
    eigenvalues are comparable; the scaled matrix is decomposed by a symmetric
    eigen-decomposition; eigen-directions whose eigenvalue is at most ``rcond``
    times the largest are dropped, and the step has no component along them
    (they stay at zero: a plane leaves its two in-plane shifts and the spin
    about its normal free); the rest is solved exactly and scaled back.
    ``rank`` is the number of directions kept; < 6 says the target does not
    constrain the pose."""
    A, b, _, _ = normal_equations(sums)
    tr_rot, tr_trans = float(np.trace(A[:3, :3])), float(np.trace(A[3:, 3:]))
    L = math.sqrt(tr_rot / tr_trans) if tr_rot > 0.0 and tr_trans > 0.0 else 1.0
    if not (L > 0.0 and math.isfinite(L)):
        L = 1.0
    s = np.array([1.0 / L] * 3 + [1.0] * 3)
    As, bs = A * s[:, None] * s[None, :], b * s
    if not (np.isfinite(As).all() and np.isfinite(bs).all()):
        return np.zeros(6), 0
    w, U = np.linalg.eigh(As)
    top = float(w[-1])
    if not top > 0.0:
        return np.zeros(6), 0
    keep = w > float(rcond) * top
    eta = (U[:, keep] * ((U[:, keep].T @ bs) / w[keep])[None, :]).sum(1)
    return eta * s, int(keep.sum())


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def compose(T, xi):
    """``exp(xi) . T`` -> 4x4 float64: the step applied on the left of ``T`` (3x4
    or 4x4).  exp is the exponential of se(3): with theta = |omega| and
    K = [omega]x, R = I + (sin theta / theta) K + ((1 - cos theta) / theta^2) K^2
    (Rodrigues) and t = (I + ((1 - cos theta) / theta^2) K +
    ((theta - sin theta) / theta^3) K^2) upsilon; below theta = 1e-6 the three
    coefficients are their series 1 - theta^2/6, 1/2 - theta^2/24 and
    1/6 - theta^2/120.  ``xi`` = 0 returns ``T`` unchanged, to the bit."""
    T = np.asarray(T, np.float64)
    out = np.eye(4)
    out[:T.shape[0]] = T
    xi = np.asarray(xi, np.float64).reshape(6)
    if not xi.any():
        return out
    w, u = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-6:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    K = _hat(w)
    K2 = K @ K
    R = np.eye(3) + a * K + b * K2
    V = np.eye(3) + b * K + c * K2
    new = np.eye(4)
    new[:3, :3] = R @ out[:3, :3]
    new[:3, 3] = R @ out[:3, 3] + V @ u
    return new


def rotation_angle(R):
    """the angle of a rotation matrix (radians), accurate near 0"""
    R = np.asarray(R, np.float64)
    s = 0.5 * math.sqrt((R[2, 1] - R[1, 2]) ** 2 + (R[0, 2] - R[2, 0]) ** 2
                        + (R[1, 0] - R[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (float(np.trace(R)) - 1.0))


# ---------------------------------------------------------------------------
# robust kernels: the scale and its schedule (host)
# ---------------------------------------------------------------------------
ROBUST_KINDS = ("none", "huber", "tukey")
_ROBUST_TUNING = {"huber": 1.345, "tukey": 4.685}


def robust_scale_for(kind: str, sigma: float) -> float:
    """The ``robust_scale`` that keeps 95 % of least squares' efficiency on
    Gaussian residuals of standard deviation ``sigma``: 1.345 sigma for "huber",
    4.685 sigma for "tukey"."""
    if kind not in _ROBUST_TUNING:
        raise ValueError(f"robust_scale_for: kind must be 'huber' or 'tukey', got {kind!r}")
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError(f"robust_scale_for: sigma must be > 0 and finite, got {sigma!r}")
    return _ROBUST_TUNING[kind] * sigma


def robust_schedule(robust: str, robust_scale, length=None):
    """``robust_scale`` (a number or a sequence) as a list of floats.  ``length``
    None: the sequence as it stands (indexed min(k, len - 1) by the TSDF loop);
    a number: exactly that many entries, a single number repeated (the levels of
    ``register_frames``).  "none" gives [None] (times ``length``)."""
    if robust not in ROBUST_KINDS:
        raise ValueError(f"robust must be one of {ROBUST_KINDS}, got {robust!r}")
    if robust == "none":
        return [None] * (1 if length is None else int(length))
    if robust_scale is None:
        raise ValueError(f"robust={robust!r} needs a robust_scale")
    scales = [float(v) for v in np.atleast_1d(np.asarray(robust_scale, np.float64)).reshape(-1)]
    if length is not None:
        if len(scales) == 1:
            scales = scales * int(length)
        if len(scales) != int(length):
            raise ValueError(f"robust_scale names {len(scales)} levels, iterations {length}")
    if not scales or not all(v > 0.0 and math.isfinite(v) for v in scales):
        raise ValueError(f"robust_scale must be > 0 and finite, got {robust_scale!r}")
    return scales


# ---------------------------------------------------------------------------
# the loop (GPU)
# ---------------------------------------------------------------------------
def _on_device(x, dtype, cols, device):
    import torch
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=dtype).reshape(-1, cols).contiguous()


def _host_step(sums, T, rcond, rows, tol_rot, tol_trans):
    """The host half of one iteration, the same in every loop: ``normal_equations``,
    ``solve_step`` and ``compose`` on the 29 doubles ``sums`` -> (the new ``T``, ``rank``,
    the keys every ``history`` entry starts from -- ``matched``, ``rmse``, ``omega``,
    ``upsilon`` --, whether the exit test held).  ``rows`` is the rows per point: 3.0 in
    mode "point", else 1.0 (a division and a product by 1.0 are exact)."""
    _, _, sse, count = normal_equations(sums)
    xi, rank = solve_step(sums, rcond)
    om, up = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
    entry = {"matched": int(round(count / rows)),
             "rmse": math.sqrt(sse * rows / count) if count > 0 else float("nan"),
             "omega": om, "upsilon": up}
    return compose(T, xi), rank, entry, bool(count > 0 and om <= tol_rot and up <= tol_trans)


def _result(T, history, rank, done, converged, n_points):
    """the dict every loop returns"""
    last = history[-1] if history else {"matched": 0, "rmse": float("nan")}
    return {"transform": T, "rmse": last["rmse"], "matched": last["matched"], "rank": rank,
            "iterations": done, "converged": converged, "history": history,
            "n_points": int(n_points)}


def register_points(points, verts, faces, init=None, max_dist: float = 0.5, iterations: int = 30,
                    mode: str = "plane", max_dist_schedule=None, tol_rot: float = 1e-6,
                    tol_trans: float = 1e-6, grid=None, sort_points: bool = True,
                    rcond: float = 1e-8, device="cuda"):
    """Align ``points`` [N,3] to the mesh ``verts`` / ``faces`` -> dict:
    ``transform`` (4x4 float64: points -> mesh frame), ``rmse`` (sqrt of the mean
    squared residual over the matched points at the last evaluated transform:
    along the normal in mode "plane", the distance in mode "point"), ``matched``
    (points with a closest point within ``max_dist`` there), ``rank`` (of the last
    solve; < 6: the target did not constrain the pose, the free directions were
    left alone and the result is still returned), ``iterations`` (solves done),
    ``converged`` (a step with |omega| <= ``tol_rot`` and |upsilon| <=
    ``tol_trans`` ended the loop) and ``history`` (per iteration a dict:
    ``matched``, ``rmse``, ``omega``, ``upsilon`` -- the step's norms -- and
    ``max_dist``, and ``sums``, the 29 doubles; the statistics are those of the
    transform the iteration started from).  The default tolerances (radians,
    scene units) sit a few float32 spacings of a room-sized coordinate above
    the floor the float32 search leaves.  ``init`` (3x4 or 4x4, default the
    identity) is where the loop starts; ``max_dist_schedule`` gives the ``max_dist`` of iteration k as its
    entry min(k, len - 1), a coarse-to-fine gate.  The triangle grid (``grid``:
    ``ops.triangle_grid``'s dict of the mesh, built here when None) and the unit
    normals are made once.  ``sort_points`` orders the points once by the cell
    of their initially moved position, so that a wave's lanes walk the same
    cells: it changes time and, through the summation tree, last bits only.
    Each iteration is ``ops.register.icp_sums``, one read of 29 doubles,
    ``solve_step`` and ``compose``.  Arrays may be numpy or torch; they are moved
    to ``device``."""
    import torch

    from .. import ops
    v = _on_device(verts, torch.float32, 3, device)
    f = _on_device(faces, torch.int32, 3, device)
    pts = _on_device(points, torch.float32, 3, v.device)
    if grid is None:
        grid = ops.triangle_grid(v, f)
    unit = ops.register.face_unit_normals(v, f)
    T = compose(np.eye(4) if init is None else np.asarray(init, np.float64), np.zeros(6))
    if sort_points and pts.shape[0]:
        pts = pts[ops.register.cell_order(grid, pts, T).long()].contiguous()
    rows = 3.0 if mode == "point" else 1.0
    schedule = [float(max_dist)] if max_dist_schedule is None else \
        [float(m) for m in max_dist_schedule]
    history, rank, converged, done = [], 0, False, 0
    for k in range(int(iterations)):
        md = schedule[min(k, len(schedule) - 1)]
        sums = ops.register.icp_sums(grid, v, f, unit, pts, T, md, mode).cpu().numpy()
        T, rank, entry, converged = _host_step(sums, T, rcond, rows, tol_rot, tol_trans)
        done = k + 1
        history.append({**entry, "max_dist": md, "sums": sums})
        if converged:
            break
    return _result(T, history, rank, done, converged, pts.shape[0])


def _mesh_arrays(mesh):
    return np.asarray(mesh["verts"], np.float32).reshape(-1, 3), \
        np.asarray(mesh["faces"], np.int32).reshape(-1, 3)


def register_meshes(src_mesh, dst_mesh, sample_density=None, seed: int = 0, device="cuda", **kw):
    """Align the mesh ``src_mesh`` to ``dst_mesh`` (``load_mesh``'s dicts: ``verts``,
    ``faces``) -> ``register_points``' dict; ``transform`` moves the source's
    vertices into the target's frame.  The source points are the source's
    vertices, or with ``sample_density`` (samples per unit area)
    ``ops.sample_mesh_surface``'s area-uniform samples with ``seed``."""
    import torch

    from .. import ops
    sv, sf = _mesh_arrays(src_mesh)
    dv, df = _mesh_arrays(dst_mesh)
    if sample_density is None:
        pts = sv
    else:
        s = ops.sample_mesh_surface(torch.as_tensor(sv).to(device),
                                    torch.as_tensor(sf).to(device), float(sample_density),
                                    seed=int(seed))
        pts = s["points"]
    return register_points(pts, dv, df, device=device, **kw)


def backproject(depth, intrinsics, stride: int = 1, depth_min: float = 0.0,
                depth_max: float = math.inf):
    """The valid pixels of a z-depth image [H,W] (a torch tensor) as points in the
    camera frame -> float32 [N,3] on its device, row-major pixel order.  Pixel
    (row i, column j) with depth z is ((j + 0.5 - cx) z / fx, (i + 0.5 - cy) z / fy,
    z): the centre convention of ``ops.get_rays`` and the camera of
    ``ops.integrate_tsdf`` (looking along +z).  Valid: finite, > 0 and within
    [``depth_min``, ``depth_max``]; every ``stride``-th row and column."""
    import torch
    fx, fy, cx, cy = [float(x) for x in intrinsics]
    d = depth.float()
    H, W = int(d.shape[0]), int(d.shape[1])
    ii = torch.arange(0, H, int(stride), device=d.device)
    jj = torch.arange(0, W, int(stride), device=d.device)
    z = d[ii][:, jj]
    x = ((jj.float() + 0.5 - cx) / fx)[None, :] * z
    y = ((ii.float() + 0.5 - cy) / fy)[:, None] * z
    ok = torch.isfinite(z) & (z > 0) & (z >= float(depth_min)) & (z <= float(depth_max))
    return torch.stack([x, y, z], -1)[ok].contiguous()


def _frame_points(d, intrinsics, stride, depth_min, depth_max, depth_filter):
    """the camera-frame points a frame is registered with: ``backproject``'s, or
    with a ``depth_filter`` those of the pixels the depth front end keeps"""
    if depth_filter is None:
        return backproject(d, intrinsics, stride, depth_min, depth_max)
    from .depth_frontend import frame_points
    # the front end's validity rule has no "> 0" of its own: keep backproject's
    return frame_points(d, intrinsics, depth_filter, stride, max(float(depth_min), 1e-6),
                        min(float(depth_max), 3.0e38))[0]


def refine_pose(depth, pose, intrinsics, grid_or_mesh, stride: int = 1, depth_min: float = 0.0,
                depth_max: float = math.inf, depth_filter=None, **kw):
    """Refine the camera-to-world ``pose`` (4x4) of one z-depth frame ``depth``
    [H,W] against a mesh -> ``register_points``' dict with ``pose`` (4x4 float64,
    the refined camera-to-world pose; the same matrix as ``transform``).  The
    valid pixels are back-projected into the camera frame (``backproject``; pose
    and ``intrinsics`` (fx, fy, cx, cy) as ``ops.integrate_tsdf`` takes them) and
    registered with ``init=pose``.  ``grid_or_mesh``: a mesh dict (``verts``,
    ``faces``), optionally carrying ``grid`` (``ops.triangle_grid``'s dict of it)
    so that a sequence of frames builds it once.  ``depth_filter`` (a
    ``utils.depth_frontend.DepthFilter``): the points are those of the filtered
    frame's pixels that the depth front end keeps; None: ``backproject``'s."""
    import torch
    device = kw.pop("device", "cuda")
    d = depth if torch.is_tensor(depth) else torch.as_tensor(np.asarray(depth, np.float32))
    pts = _frame_points(d.to(device), intrinsics, stride, depth_min, depth_max, depth_filter)
    out = register_points(pts, grid_or_mesh["verts"], grid_or_mesh["faces"], init=pose,
                          grid=grid_or_mesh.get("grid"), device=device, **kw)
    out["pose"] = out["transform"]
    return out


def refine_poses(depths, poses, intrinsics, grid_or_mesh, **kw):
    """``refine_pose`` frame by frame -> list of its dicts.  The triangle grid is
    built once."""
    import torch

    from .. import ops
    device = kw.get("device", "cuda")
    mesh = dict(grid_or_mesh)
    if mesh.get("grid") is None:
        mesh["verts"] = _on_device(mesh["verts"], torch.float32, 3, device)
        mesh["faces"] = _on_device(mesh["faces"], torch.int32, 3, device)
        mesh["grid"] = ops.triangle_grid(mesh["verts"], mesh["faces"])
    return [refine_pose(d, p, intrinsics, mesh, **kw) for d, p in zip(depths, poses)]


# ---------------------------------------------------------------------------
# against a TSDF volume: frame-to-model tracking
# ---------------------------------------------------------------------------
def register_points_tsdf(points, volume, trunc: float, init=None, iterations: int = 30,
                         min_weight: float = 1.0, max_tsdf: float = 1.0, max_tsdf_schedule=None,
                         tol_rot: float = 1e-6, tol_trans: float = 1e-6, rcond: float = 1e-8,
                         device="cuda", robust: str = "none", robust_scale=None,
                         point_weight=None):
    """Align ``points`` [N,3] to the surface a TSDF ``volume`` holds
    (``ops.tsdf_volume``'s dict on the device, integrated with the truncation
    distance ``trunc``) -> ``register_points``' dict with the same keys
    (``history`` entries carry ``max_tsdf`` in place of ``max_dist``).  No mesh
    is extracted and nothing is searched: the residual of a moved point q is the
    volume's trilinear signed distance there, r = -(F * trunc), and its normal
    n the normalised gradient, pointing toward free space; the surface point is
    q - F trunc n, so r has the sign of the mesh route's n . (c - q) and
    ``solve_step`` / ``compose`` are used unchanged.  Each iteration is
    ``ops.register.tsdf_sums``, one read of 29 doubles, ``solve_step`` and
    ``compose``.  A point matches where all eight corners of its cell have
    weight >= ``min_weight`` and |F| <= ``max_tsdf`` (units of ``trunc``, at
    most 1); ``max_tsdf_schedule`` gives the gate of iteration k as its entry
    min(k, len - 1), coarse to fine, like ``max_dist_schedule``.

    The basin: the volume carries signal only within ``trunc`` of a surface --
    beyond it F is clamped to +-1, the gradient is zero and nothing matches --
    so the pose error, measured at the surface (translation plus angle times
    the distance to the surface), must stay below ``trunc``.  Anything coarser
    is the mesh route's job (``register_points`` with a ``max_dist_schedule``)
    or global alignment (``global_register_points_tsdf``).

    ``robust`` ("none", "huber", "tukey"), ``robust_scale`` and ``point_weight``
    turn the loop into iteratively reweighted least squares: each iteration is
    then ``ops.register.tsdf_sums_weighted`` with the kernel, the scale of
    iteration k -- ``robust_scale`` is a number, or a sequence indexed
    min(k, len - 1) like ``max_tsdf_schedule``, in scene units like r --
    and ``point_weight`` [N] (a weight per point, float32; a point whose weight
    is not finite and > 0 takes no part).  ``matched`` then counts the rows with
    a positive weight, ``rmse`` is sqrt(sum w r^2 / that count), and every
    ``history`` entry carries ``robust`` and ``robust_scale``.  With the defaults
    the loop calls ``tsdf_sums`` and nothing else, and its entries have no such
    keys.  For tracking, from a pose already near the answer: "tukey" ignores
    what lies beyond its scale, true matches of a far start included."""
    import torch

    from .. import ops
    pts = _on_device(points, torch.float32, 3, device)
    T = compose(np.eye(4) if init is None else np.asarray(init, np.float64), np.zeros(6))
    schedule = [float(max_tsdf)] if max_tsdf_schedule is None else \
        [float(m) for m in max_tsdf_schedule]
    scales = robust_schedule(robust, robust_scale)
    weighted = robust != "none" or point_weight is not None
    pw = None if point_weight is None else \
        _on_device(point_weight, torch.float32, 1, pts.device).reshape(-1)
    history, rank, converged, done = [], 0, False, 0
    for k in range(int(iterations)):
        mt = schedule[min(k, len(schedule) - 1)]
        extra = {}
        if weighted:
            sc = scales[min(k, len(scales) - 1)]
            sums = ops.register.tsdf_sums_weighted(volume, pts, T, trunc, min_weight, mt, pw,
                                                   robust, sc).cpu().numpy()
            extra = {"robust": robust, "robust_scale": sc}
        else:
            sums = ops.register.tsdf_sums(volume, pts, T, trunc, min_weight, mt).cpu().numpy()
        T, rank, entry, converged = _host_step(sums, T, rcond, 1.0, tol_rot, tol_trans)
        done = k + 1
        history.append({**entry, "max_tsdf": mt, "sums": sums, **extra})
        if converged:
            break
    return _result(T, history, rank, done, converged, pts.shape[0])


def _float_rows(T):
    """float64 [K,3,4] or [K,4,4] -> the float32 rows [K,3,4] a kernel reads: the
    rounding of ``ops.register``'s ``_transform12``"""
    T = np.asarray(T, np.float64)
    return np.ascontiguousarray(T.reshape(-1, T.shape[-2], 4)[:, :3].astype(np.float32))


def lockstep_loop(sums_fn, inits, iterations: int = 30, max_tsdf: float = 1.0,
                  max_tsdf_schedule=None, tol_rot: float = 1e-6, tol_trans: float = 1e-6,
                  rcond: float = 1e-8, n_points: int = 0):
    """``register_points_tsdf``'s loop for K starts ``inits`` (4x4 or 3x4 each) in
    lock step, over ``sums_fn(transforms, max_tsdf)``: float32 [A,3,4] (the still
    active hypotheses' transforms, rounded as the single loop rounds them) and
    the iteration's gate -> float64 [A,29], row a what ``tsdf_sums`` gives for
    transform a -> a list of K dicts, each what the single loop returns for its
    start.  Host arithmetic only: per row the same ``normal_equations``,
    ``solve_step`` and ``compose`` calls as the single loop, one row after
    another (a batched eigen-decomposition need not give the same bits), so
    with a ``sums_fn`` whose rows are exact the results are equal bit for bit.
    A hypothesis that meets its exit test leaves the active set; ``sums_fn`` is
    called once per iteration while any is active."""
    T = [compose(np.asarray(t, np.float64), np.zeros(6)) for t in inits]
    K = len(T)
    schedule = [float(max_tsdf)] if max_tsdf_schedule is None else \
        [float(m) for m in max_tsdf_schedule]
    history = [[] for _ in range(K)]
    rank, converged, done = [0] * K, [False] * K, [0] * K
    active = list(range(K))
    for k in range(int(iterations)):
        if not active:
            break
        mt = schedule[min(k, len(schedule) - 1)]
        rows = np.asarray(sums_fn(_float_rows(np.stack([T[j] for j in active])), mt), np.float64)
        if rows.shape != (len(active), SUMS):
            raise ValueError(f"sums_fn must return [{len(active)},{SUMS}], got {rows.shape}")
        still = []
        for a, j in enumerate(active):
            sums = rows[a].copy()
            T[j], rank[j], entry, converged[j] = _host_step(sums, T[j], rcond, 1.0, tol_rot,
                                                            tol_trans)
            done[j] = k + 1
            history[j].append({**entry, "max_tsdf": mt, "sums": sums})
            if not converged[j]:
                still.append(j)
        active = still
    return [_result(T[j], history[j], rank[j], done[j], converged[j], n_points) for j in range(K)]


def register_points_tsdf_batch(points, volume, trunc: float, inits, iterations: int = 30,
                               min_weight: float = 1.0, max_tsdf: float = 1.0,
                               max_tsdf_schedule=None, tol_rot: float = 1e-6,
                               tol_trans: float = 1e-6, rcond: float = 1e-8, device="cuda",
                               sums_fn=None):
    """``register_points_tsdf`` from K starts ``inits`` ([K,4,4] or a sequence of
    4x4 / 3x4) in lock step -> a list of K dicts, entry k exactly -- keys, values
    and bits: ``transform``, every ``history[i]["sums"]``, ``iterations``,
    ``converged``, ``matched``, ``rank``, ``rmse`` -- what
    ``register_points_tsdf(points, volume, trunc, init=inits[k], ...)`` returns.
    Each iteration is one ``ops.register.tsdf_sums_batch`` call for all
    hypotheses still active (their float64 transforms rounded to float32 and
    uploaded in one copy), one read of [active, 29] doubles, and per row the
    single loop's host step; a hypothesis that converges leaves the batch.  K
    loops then cost max(iterations) launches and reads, not their sum.
    ``max_tsdf_schedule`` is indexed by the iteration, which all active
    hypotheses share.  At most ``ops.register.TSDF_SUMS_BATCH_MAX`` starts.
    ``sums_fn`` replaces the device call (``lockstep_loop``'s argument; then
    ``points`` and ``volume`` are only counted, and no GPU is needed)."""
    if sums_fn is None:
        import torch

        from .. import ops
        pts = _on_device(points, torch.float32, 3, device)
        n = int(pts.shape[0])

        def sums_fn(rows, mt):
            T = torch.from_numpy(rows).to(pts.device)
            return ops.register.tsdf_sums_batch(volume, pts, T, trunc, min_weight,
                                                mt).cpu().numpy()
    else:
        n = int(np.asarray(points).reshape(-1, 3).shape[0])
    return lockstep_loop(sums_fn, list(inits), iterations, max_tsdf, max_tsdf_schedule, tol_rot,
                         tol_trans, rcond, n_points=n)


def refine_pose_tsdf(depth, pose, intrinsics, volume, trunc: float, stride: int = 1,
                     depth_min: float = 0.0, depth_max: float = math.inf, depth_filter=None,
                     **kw):
    """Refine the camera-to-world ``pose`` (4x4) of one z-depth frame ``depth``
    [H,W] against the TSDF ``volume`` as it stands -> ``register_points_tsdf``'s
    dict with ``pose`` (4x4 float64, the same matrix as ``transform``).  The
    valid pixels are back-projected into the camera frame (``backproject``) and
    registered with ``init=pose``: frame-to-model tracking, for a pose whose
    error at the surface is below ``trunc`` (see ``register_points_tsdf``).
    ``depth_filter`` as for ``refine_pose``.  ``robust``, ``robust_scale`` and
    ``point_weight`` (one weight per point kept, in ``backproject``'s row-major
    order) go to ``register_points_tsdf`` with the rest of ``kw``."""
    import torch
    device = kw.pop("device", "cuda")
    d = depth if torch.is_tensor(depth) else torch.as_tensor(np.asarray(depth, np.float32))
    pts = _frame_points(d.to(device), intrinsics, stride, depth_min, depth_max, depth_filter)
    out = register_points_tsdf(pts, volume, trunc, init=pose, device=device, **kw)
    out["pose"] = out["transform"]
    return out


def pose_step(a, b):
    """the difference of two 4x4 poses -> (radians, units): the angle of the
    relative rotation and the distance of the camera centres"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return rotation_angle(a[:3, :3] @ b[:3, :3].T), float(np.linalg.norm(a[:3, 3] - b[:3, 3]))


# ---------------------------------------------------------------------------
# projective association: frame to frame and frame to model
# ---------------------------------------------------------------------------
_NORMAL, _EDGE, _GRAZING = 2, 4, 8


def level_intrinsics(intrinsics, level: int):
    """(fx, fy, cx, cy) of pyramid level ``level``: each divided by 2^level, exact
    under the +0.5 pixel-centre convention (coarse pixel J covers [2J, 2J + 2))"""
    s = 2.0 ** int(level)
    return tuple(float(v) / s for v in intrinsics)


def frame_maps(depth, intrinsics, depth_filter=None, levels: int = 3, filtered=None,
               depth_min: float = 1e-6, depth_max: float = 3.0e38, device="cuda"):
    """The vertex and normal maps of one z-depth frame ``depth`` [H,W] on a depth
    pyramid -> list over the levels, finest first, of dicts: ``depth`` [h,w],
    ``points`` and ``normals`` [h,w,3] float32 in the camera frame, ``mask`` [h,w]
    uint8 (``ops.depth.depth_normals``' bits) and ``intrinsics``
    (``level_intrinsics``), all on the device.  Level 0 is the frame itself --
    through the bilateral filter when a ``depth_filter`` (a
    ``utils.depth_frontend.DepthFilter``) is given (``filtered`` overrides that
    choice) -- and level l + 1 is ``ops.depth.pyramid_down`` of level l.  The
    thresholds are the filter's (None: its defaults) with ``max_jump`` and
    ``max_jump_z2`` multiplied by 2^level at level ``level``: a coarse pixel is
    2^level times as wide, so the depth step between neighbours on a slanted
    surface grows as much, and with the fine threshold the coarse levels lose
    their normals."""
    import torch

    from .. import ops
    from .depth_frontend import DepthFilter, run_frontend
    flt = DepthFilter() if depth_filter is None else depth_filter
    filtered = depth_filter is not None if filtered is None else bool(filtered)
    d = depth if torch.is_tensor(depth) else torch.as_tensor(np.array(depth, np.float32))
    d = d.to(device=device, dtype=torch.float32)[None].contiguous()
    out = []
    for level in range(int(levels)):
        s = 2.0 ** level
        K = level_intrinsics(intrinsics, level)
        if level == 0 and filtered:
            m = run_frontend(d, K, flt, depth_min, depth_max)
            d = m["depth"]
        else:
            if level:
                d = ops.depth.pyramid_down(d, flt.max_jump * (s / 2), flt.max_jump_z2 * (s / 2),
                                           depth_min, depth_max)
            m = ops.depth.depth_normals(d, K, flt.max_jump * s, flt.max_jump_z2 * s, flt.min_cos,
                                        depth_min, depth_max)
        out.append({"depth": d[0], "points": m["points"][0], "normals": m["normals"][0],
                    "mask": m["mask"][0], "intrinsics": K})
    return out


def _source_rows(maps, reject):
    """the pixels of one level a frame is registered with: those with a normal and
    no bit of ``reject``, in row-major order -> (points [N,3], normals [N,3])"""
    m = maps["mask"]
    keep = ((m & _NORMAL) != 0) & ((m & reject) == 0)
    return maps["points"][keep].contiguous(), maps["normals"][keep].contiguous()


def _source_weights(maps, reject, level_weight, view_weights, depth_filter):
    """the weights of ``_source_rows``' rows -> float32 [N] or None: the map
    ``level_weight`` [h,w], or ``ops.depth.depth_confidence`` of the level's maps
    with the settings ``view_weights``, at the kept pixels"""
    import torch

    from .. import ops
    if level_weight is None and view_weights is None:
        return None
    m = maps["mask"]
    keep = ((m & _NORMAL) != 0) & ((m & reject) == 0)
    if view_weights is not None:
        from .depth_frontend import DepthFilter
        sd, s2 = view_weights.resolved(DepthFilter() if depth_filter is None else depth_filter)
        w = ops.depth.depth_confidence(maps["points"][None], maps["normals"][None], m[None], sd,
                                       s2, view_weights.cos_floor, reject)[0]
    else:
        w = level_weight if torch.is_tensor(level_weight) else \
            torch.as_tensor(np.asarray(level_weight, np.float32))
        w = w.to(device=m.device, dtype=torch.float32)
        if tuple(w.shape) != tuple(m.shape):
            raise ValueError(f"point_weight of a level must be {tuple(m.shape)}, got "
                             f"{tuple(w.shape)}")
    return w[keep].contiguous()


def register_frames(src_maps, dst_maps, intrinsics, init=None, iterations=(10, 5, 4),
                    max_dist: float = 0.3, min_cos: float = 0.8, reject: int = _EDGE | _GRAZING,
                    rcond: float = 1e-8, tol_rot: float = 1e-6, tol_trans: float = 1e-6,
                    robust: str = "none", robust_scale=None, point_weight=None,
                    view_weights=None, depth_filter=None):
    """Align one frame to a second pair of maps by projective point-to-plane ICP,
    coarse to fine -> ``register_points``' dict; ``transform`` (4x4 float64) moves
    the source camera's frame into the target camera's, and every ``history``
    entry carries its ``level``.  ``src_maps`` and ``dst_maps`` are
    ``frame_maps``' lists (the target may also be a model view dressed the same
    way: ``refine_pose_projective``); ``intrinsics`` (fx, fy, cx, cy) of level 0.
    ``iterations`` gives the iterations per level, finest first, and the number
    of levels: (10, 5, 4) runs 4 at level 2, then 5 at level 1, then 10 at level
    0; ``(n,)`` is a single level.  A level ends early on a step with |omega| <=
    ``tol_rot`` and |upsilon| <= ``tol_trans``.  The source points of a level are
    its pixels with a normal and no bit of ``reject``; a pair matches within
    ``max_dist`` and with a cosine of the normals >= ``min_cos``.  Each iteration
    is ``ops.register.projective_sums``, one read of 29 doubles, ``solve_step``
    and ``compose``.  The basin is set by ``max_dist`` and the scene, not by a
    truncation band; rank < 6 says the views do not constrain the motion.

    ``robust`` ("none", "huber", "tukey") with ``robust_scale`` -- a number, or
    one per level, finest first, like ``iterations``; in scene units like r --
    and a weight per source pixel turn the loop into iteratively reweighted
    least squares: each iteration is then
    ``ops.register.projective_sums_weighted``.  The pixel weights are
    ``point_weight``, a sequence over the levels, finest first, of [h,w] float32
    maps (None for a level without; a single map where there is one level), or
    with ``view_weights`` (a ``utils.depth_frontend.ViewWeights``; its None
    sigmas are ``depth_filter``'s, None: the defaults')
    ``ops.depth.depth_confidence`` of the source level's own maps; a source row
    takes the value at its pixel, and one that is not finite and > 0 takes no
    part.  ``matched`` then counts the rows with a positive weight, ``rmse`` is
    sqrt(sum w r^2 / that count), and every ``history`` entry carries ``robust``
    and ``robust_scale``.  With the defaults the loop calls ``projective_sums``
    and nothing else, and its entries have no such keys.  This is for tracking,
    from a few degrees and centimetres: "tukey" ignores what lies beyond its
    scale, true matches of a far start included, and a scale widened on the
    coarse levels can lock onto the outliers instead (docs/DESIGN_NOTEBOOK.md,
    section RB)."""
    from .. import ops
    iterations = tuple(int(k) for k in iterations)
    if not iterations or len(src_maps) < len(iterations) or len(dst_maps) < len(iterations):
        raise ValueError(f"iterations names {len(iterations)} levels, the maps have "
                         f"{len(src_maps)} and {len(dst_maps)}")
    scales = robust_schedule(robust, robust_scale, len(iterations))
    if point_weight is not None and view_weights is not None:
        raise ValueError("give point_weight or view_weights, not both")
    if point_weight is not None and not isinstance(point_weight, (list, tuple)):
        point_weight = [point_weight]
    if point_weight is not None and len(point_weight) != len(iterations):
        raise ValueError(f"point_weight names {len(point_weight)} levels, iterations "
                         f"{len(iterations)}")
    weighted = robust != "none" or point_weight is not None or view_weights is not None
    T = compose(np.eye(4) if init is None else np.asarray(init, np.float64), np.zeros(6))
    history, rank, done, converged, n_points = [], 0, 0, False, 0
    for level in reversed(range(len(iterations))):
        pts, nrm = _source_rows(src_maps[level], reject)
        dst = dst_maps[level]
        K = level_intrinsics(intrinsics, level)
        n_points, converged = int(pts.shape[0]), False
        extra = {}
        if weighted:
            pw = _source_weights(src_maps[level], reject,
                                 None if point_weight is None else point_weight[level],
                                 view_weights, depth_filter)
            extra = {"robust": robust, "robust_scale": scales[level]}
        for _ in range(iterations[level]):
            if weighted:
                sums = ops.register.projective_sums_weighted(
                    pts, nrm, dst["points"], dst["normals"], dst["mask"], K, T, max_dist, min_cos,
                    reject, pw, robust, scales[level]).cpu().numpy()
            else:
                sums = ops.register.projective_sums(pts, nrm, dst["points"], dst["normals"],
                                                    dst["mask"], K, T, max_dist, min_cos,
                                                    reject).cpu().numpy()
            T, rank, entry, converged = _host_step(sums, T, rcond, 1.0, tol_rot, tol_trans)
            done += 1
            history.append({"level": level, **entry, "max_dist": float(max_dist), "sums": sums,
                            **extra})
            if converged:
                break
    return _result(T, history, rank, done, converged, n_points)


def odometry(depths, intrinsics, depth_filter=None, iterations=(10, 5, 4),
             min_matched: float = 0.25, filtered=None, device="cuda", **kw):
    """Camera poses of a depth sequence without any given pose: ``register_frames``
    of every frame to the one before it, chained -> dict: ``poses`` [N,4,4]
    float64 camera-to-world with frame 0 at the identity, ``records`` (per pair
    a dict: ``matched`` -- the share of the source points --, ``rmse``, ``rank``,
    ``iterations``, ``fallback``; None for frame 0) and ``fallbacks``.  A pair
    whose last solve has rank < 6 or whose matched share is below
    ``min_matched`` falls back: its motion is kept at the identity and counted.
    Frame to frame: the drift adds up; fuse and track against the model
    (``refine_pose_projective``) where a volume is at hand.  ``depth_filter`` and
    ``filtered`` are ``frame_maps``'; ``kw`` goes to ``register_frames``:
    ``robust``, ``robust_scale``, ``point_weight`` and ``view_weights`` among it
    (the latter resolved against ``depth_filter``)."""
    levels = len(tuple(iterations))
    if kw.get("view_weights") is not None:
        kw.setdefault("depth_filter", depth_filter)
    poses, records, fallbacks, prev = [np.eye(4)], [None], 0, None
    for d in depths:
        maps = frame_maps(d, intrinsics, depth_filter, levels, filtered, device=device)
        if prev is not None:
            out = register_frames(maps, prev, intrinsics, iterations=iterations, **kw)
            share = out["matched"] / out["n_points"] if out["n_points"] else 0.0
            fallback = bool(out["rank"] < 6 or share < min_matched)
            fallbacks += fallback
            poses.append(poses[-1] @ (np.eye(4) if fallback else out["transform"]))
            records.append({"matched": share, "rmse": out["rmse"], "rank": out["rank"],
                            "iterations": out["iterations"], "fallback": fallback})
        prev = maps
    return {"poses": np.stack(poses), "records": records, "fallbacks": int(fallbacks)}


def model_maps(volume, pose, intrinsics, sizes, trunc: float, near: float, far: float,
               min_weight: float = 1.0):
    """The model seen from the camera-to-world ``pose`` as target maps, one dict per
    level of ``sizes`` [(h, w), ...] in ``frame_maps``' layout: the depth of
    ``ops.raycast_tsdf`` with the level's intrinsics, its back-projection
    (``ops.depth.depth_normals``' points), the ray-caster's world-frame normals
    rotated into the camera frame (n_k = (R[0][k] n0 + R[1][k] n1) + R[2][k] n2,
    elementwise float32) and mask 3 (measured, normal) where the normal is not
    zero, 0 elsewhere."""
    import torch

    from .. import ops
    dev = volume["tsdf"].device
    P = torch.as_tensor(np.asarray(pose, np.float64)).to(torch.float32).to(dev)
    out = []
    for level, (h, w) in enumerate(sizes):
        K = level_intrinsics(intrinsics, level)
        rc = ops.raycast_tsdf(volume, P[None], K, int(h), int(w), near, far, trunc=trunc,
                              min_weight=min_weight)
        nw = rc["normal"][0]
        points = ops.depth.depth_normals(rc["depth"], K, 0.0, 0.0, 0.0)["points"][0]
        nc = torch.stack([(P[0, k] * nw[..., 0] + P[1, k] * nw[..., 1]) + P[2, k] * nw[..., 2]
                          for k in range(3)], -1).contiguous()
        mask = ((nw != 0).any(-1).to(torch.uint8) * 3).contiguous()
        out.append({"depth": rc["depth"][0], "points": points, "normals": nc, "mask": mask,
                    "intrinsics": K})
    return out


def refine_pose_projective(depth, pose, intrinsics, volume, trunc: float, iterations=(10,),
                           near: float = 0.05, far: float = 100.0, min_weight: float = 1.0,
                           depth_filter=None, filtered=None, depth_min: float = 1e-6,
                           depth_max: float = 3.0e38, **kw):
    """Refine the camera-to-world ``pose`` (4x4) of one z-depth frame ``depth``
    [H,W] against the TSDF ``volume`` by projective ICP -> ``register_frames``'
    dict with ``pose`` (4x4 float64) = ``pose`` . ``transform``.  The target
    maps are the model ray-cast once from ``pose`` at every level
    (``model_maps``; ``near`` / ``far`` bound the cast), the source maps are
    ``frame_maps`` of the frame, and ``transform`` starts at the identity: the
    motion from the frame's true camera to the camera at ``pose``.  Unlike
    ``refine_pose_tsdf`` the pose error at the surface may exceed ``trunc``: the
    gate is ``register_frames``' ``max_dist``.  ``depth_filter`` and ``filtered``
    are ``frame_maps``'; ``kw`` goes to ``register_frames``: ``robust``,
    ``robust_scale``, ``point_weight`` and ``view_weights`` among it (the latter
    resolved against ``depth_filter``)."""
    iterations = tuple(int(k) for k in iterations)
    if kw.get("view_weights") is not None:
        kw.setdefault("depth_filter", depth_filter)
    dev = volume["tsdf"].device
    src = frame_maps(depth, intrinsics, depth_filter, len(iterations), filtered,
                     depth_min=depth_min, depth_max=depth_max, device=dev)
    sizes = [tuple(m["mask"].shape) for m in src]
    dst = model_maps(volume, pose, intrinsics, sizes, trunc, near, far, min_weight)
    out = register_frames(src, dst, intrinsics, iterations=iterations, **kw)
    out["pose"] = np.asarray(pose, np.float64) @ out["transform"]
    return out


# ---------------------------------------------------------------------------
# global alignment: many hypotheses scored against a TSDF volume
# ---------------------------------------------------------------------------
_SF_PHI = math.sqrt(2.0)
_SF_PSI = 1.533751168755204288118041


def rotation_set(n: int):
    """``n`` rotations spread evenly over SO(3) -> float64 [n,3,3], deterministic:
    the super-Fibonacci spiral (Alexa 2022).  With s = i + 1/2, the unit
    quaternion i is (sqrt(s/n) sin a, sqrt(s/n) cos a, sqrt(1 - s/n) sin b,
    sqrt(1 - s/n) cos b) with a = 2 pi s / sqrt(2) and b = 2 pi s / psi,
    psi = 1.5337511687552043 (the root of psi^4 = psi + 4).  Host, numpy; the
    covering angle of ``rotation_set(4096)`` is measured in
    tests/test_global_register_cpu.py."""
    n = int(n)
    if n < 1:
        raise ValueError(f"rotation_set needs n >= 1, got {n}")
    s = np.arange(n, dtype=np.float64) + 0.5
    r, R = np.sqrt(s / n), np.sqrt(1.0 - s / n)
    a, b = 2.0 * math.pi * s / _SF_PHI, 2.0 * math.pi * s / _SF_PSI
    x, y, z, w = r * np.sin(a), r * np.cos(a), R * np.sin(b), R * np.cos(b)
    out = np.empty((n, 3, 3), np.float64)
    out[:, 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    out[:, 0, 1] = 2.0 * (x * y - z * w)
    out[:, 0, 2] = 2.0 * (x * z + y * w)
    out[:, 1, 0] = 2.0 * (x * y + z * w)
    out[:, 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    out[:, 1, 2] = 2.0 * (y * z - x * w)
    out[:, 2, 0] = 2.0 * (x * z - y * w)
    out[:, 2, 1] = 2.0 * (y * z + x * w)
    out[:, 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return out


def surface_centroid(volume, trunc: float, min_weight: float = 1.0):
    """The mean position of the voxels of a TSDF ``volume`` (numpy arrays or
    tensors on any device) that lie within one voxel of its surface: weight >=
    ``min_weight`` and |tsdf| * ``trunc`` <= the largest spacing, both in
    float32 -> float64 [3].  The voxels' indices are summed as integers, so the
    result is the same to the bit wherever the volume lives."""
    tsdf, weight = volume["tsdf"], volume["weight"]
    o = np.asarray(volume["origin"], np.float32).astype(np.float64).reshape(3)
    h32 = np.broadcast_to(np.asarray(volume["spacing"], np.float32), (3,))
    voxel, tr, mw = float(h32.max()), float(np.float32(trunc)), float(np.float32(min_weight))
    if hasattr(tsdf, "detach"):                       # a tensor
        band = (weight >= mw) & (tsdf.abs() * tr <= voxel)
        idx = band.nonzero()
        count, total = int(idx.shape[0]), idx.sum(0).cpu().numpy().astype(np.int64)
    else:
        t32, w32 = np.asarray(tsdf, np.float32), np.asarray(weight, np.float32)
        band = (w32 >= np.float32(mw)) & (np.abs(t32) * np.float32(tr) <= np.float32(voxel))
        idx = np.argwhere(band)
        count, total = int(idx.shape[0]), idx.sum(0, dtype=np.int64)
    if count == 0:
        raise ValueError("surface_centroid: the volume holds no surface voxel")
    return o + (total.astype(np.float64) / float(count)) * h32.astype(np.float64)


def hypotheses(rotations, src_centroid, dst_centroid, offsets=None):
    """Rigid hypotheses [R | t] -> float64 [K,3,4]: every rotation of ``rotations``
    [n,3,3] with the translation that moves ``src_centroid`` onto
    ``dst_centroid`` + offset, t = dst_centroid + offset - R . src_centroid.
    ``offsets`` [M,3] (None: the one offset 0) multiplies K by M, for point sets
    that overlap the target only partly; hypothesis r * M + m is rotation r with
    offset m."""
    R = np.asarray(rotations, np.float64).reshape(-1, 3, 3)
    off = np.zeros((1, 3)) if offsets is None else np.asarray(offsets, np.float64).reshape(-1, 3)
    src = np.asarray(src_centroid, np.float64).reshape(3)
    dst = np.asarray(dst_centroid, np.float64).reshape(3)
    out = np.empty((R.shape[0], off.shape[0], 3, 4), np.float64)
    out[..., :3] = R[:, None]
    out[..., 3] = (dst + off)[None, :, :] - (R @ src)[:, None, :]
    return out.reshape(-1, 3, 4)


def rank_scores(scores):
    """The order of ``ops.register.tsdf_scores``' rows [K,4], best first: inliers -
    free descending, then sum e^2 ascending, then the index -> int64 [K]."""
    s = np.asarray(scores, np.int64).reshape(-1, 4)
    return np.lexsort((np.arange(s.shape[0]), s[:, 3], -(s[:, 0] - s[:, 1]))).astype(np.int64)


def transform_distance(a, b, at):
    """(radians, units) between two rigid transforms: the angle of the relative
    rotation and how far apart they put the point ``at``"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    at = np.asarray(at, np.float64).reshape(3)
    return rotation_angle(a[:3, :3] @ b[:3, :3].T), \
        float(np.linalg.norm((a[:3, :3] @ at + a[:3, 3]) - (b[:3, :3] @ at + b[:3, 3])))


def is_ambiguous(candidates, src_centroid, n_points: int, trunc: float,
                 ambiguity_share: float = 0.02, min_angle: float = 0.1):
    """``candidates`` (dicts with ``transform`` and ``score``, best first): does one
    farther than (``min_angle`` rad or ``trunc`` units at the source's centroid)
    from the first have a key inliers - free within ``ambiguity_share`` of the
    points of the first's?"""
    if not candidates:
        return False
    key = lambda c: int(c["score"][0]) - int(c["score"][1])
    best = candidates[0]
    for c in candidates[1:]:
        rot, trans = transform_distance(c["transform"], best["transform"], src_centroid)
        if (rot > min_angle or trans > trunc) and \
                key(best) - key(c) <= ambiguity_share * n_points:
            return True
    return False


def global_register_points_tsdf(points, volume, trunc: float, coarse=None, coarse_trunc=None,
                                n_rotations: int = 4096, offsets=None, keep: int = 16,
                                max_tsdf: float = 0.75, coarse_iterations: int = 10,
                                fine_iterations: int = 15, min_weight: float = 1.0,
                                ambiguity_share: float = 0.02, rotations=None, device="cuda",
                                lockstep: bool = False):
    """Align ``points`` [N,3] to the surface a TSDF ``volume`` holds from an unknown
    pose: a search over rotations, not a refinement -> ``register_points_tsdf``'s
    dict of the winner plus ``score`` (its four integers of
    ``ops.register.tsdf_scores`` on ``volume``), ``n_hypotheses``, ``candidates``
    (the refined hypotheses, best first: dicts with ``index``, ``transform``,
    ``score``, ``coarse_score``) and ``ambiguous``.

    1. ``hypotheses`` of ``rotation_set(n_rotations)`` (or ``rotations`` [n,3,3]),
       the centroid of the finite points and ``surface_centroid`` of the coarse
       volume, times ``offsets``, are scored in one ``tsdf_scores`` call on
       ``coarse`` (a volume of the same surface with a wider band,
       ``coarse_trunc``; None: ``volume`` itself) with the gate ``max_tsdf``.
    2. They are ordered by ``rank_scores``: inliers - free, then sum e^2.  A point
       that lands where the volume saw empty space counts against a hypothesis:
       that is what tells a room's symmetric poses apart.
    3. The first ``keep`` are refined by ``register_points_tsdf``:
       ``coarse_iterations`` on the coarse volume, then ``fine_iterations`` on
       ``volume``.  With ``lockstep`` the two phases are each one
       ``register_points_tsdf_batch`` over all kept hypotheses (at most
       ``ops.register.TSDF_SUMS_BATCH_MAX`` of them): one launch and one read
       per iteration instead of one per hypothesis and iteration.  The phases
       are independent per hypothesis either way and the returned dict is
       equal bit for bit.
    4. The refined transforms are scored on ``volume`` in one call and ordered
       the same way; the first wins.

    ``ambiguous`` (``is_ambiguous``): a candidate elsewhere -- more than 0.1 rad
    or ``trunc`` away -- scores within ``ambiguity_share`` of the points of the
    winner: a symmetric target, and the winner is one of several answers.  The
    set's covering angle must lie inside the coarse loop's basin; the figures for
    4 096 rotations are in docs/DESIGN_NOTEBOOK.md, section GR."""
    import torch

    from .. import ops
    pts = _on_device(points, torch.float32, 3, device)
    if coarse is None:
        coarse, coarse_trunc = volume, trunc
    elif coarse_trunc is None:
        raise ValueError("a coarse volume needs its coarse_trunc")
    host = pts.cpu().numpy().astype(np.float64)
    host = host[np.isfinite(host).all(1)]
    if host.shape[0] == 0:
        raise ValueError("global_register_points_tsdf: no finite point")
    src_c = host.mean(0)
    R = rotation_set(n_rotations) if rotations is None else rotations
    H = hypotheses(R, src_c, surface_centroid(coarse, coarse_trunc, min_weight), offsets)
    to_dev = lambda a: torch.from_numpy(a).to(pts.device)
    first = ops.register.tsdf_scores(coarse, pts, to_dev(_float_rows(H)), min_weight,
                                     max_tsdf).cpu().numpy()
    refined = []
    kept = rank_scores(first)[:int(keep)]
    if lockstep:
        outs = register_points_tsdf_batch(pts, coarse, coarse_trunc, [H[k] for k in kept],
                                          iterations=coarse_iterations, min_weight=min_weight,
                                          device=pts.device)
        outs = register_points_tsdf_batch(pts, volume, trunc, [o["transform"] for o in outs],
                                          iterations=fine_iterations, min_weight=min_weight,
                                          device=pts.device)
        refined = [(int(k), o) for k, o in zip(kept, outs)]
    else:
        for k in kept:
            out = register_points_tsdf(pts, coarse, coarse_trunc, init=H[k],
                                       iterations=coarse_iterations, min_weight=min_weight,
                                       device=pts.device)
            out = register_points_tsdf(pts, volume, trunc, init=out["transform"],
                                       iterations=fine_iterations, min_weight=min_weight,
                                       device=pts.device)
            refined.append((int(k), out))
    last = ops.register.tsdf_scores(
        volume, pts, to_dev(_float_rows(np.stack([o["transform"] for _, o in refined]))),
        min_weight, max_tsdf).cpu().numpy()
    order = rank_scores(last)
    candidates = [{"index": refined[j][0], "transform": refined[j][1]["transform"],
                   "score": tuple(int(v) for v in last[j]),
                   "coarse_score": tuple(int(v) for v in first[refined[j][0]])} for j in order]
    result = dict(refined[int(order[0])][1])
    result.update(score=candidates[0]["score"], n_hypotheses=int(H.shape[0]),
                  candidates=candidates,
                  ambiguous=is_ambiguous(candidates, src_c, int(pts.shape[0]), float(trunc),
                                         ambiguity_share))
    return result


def global_register_meshes(src_mesh, dst_mesh, voxel: float, trunc=None, coarse_factor: float = 3,
                           samples: int = 2048, seed: int = 0, device="cuda", **kw):
    """Align the mesh ``src_mesh`` to ``dst_mesh`` (``load_mesh``'s dicts) from an
    unknown pose -> ``global_register_points_tsdf``'s dict; ``transform`` moves
    the source's vertices into the target's frame.  The fine volume is
    ``utils.tsdf_fusion.volume_from_mesh`` of the target at ``voxel`` and
    ``trunc`` (default 4 voxels), the coarse one the same at ``coarse_factor``
    times both.  The source points are about ``samples`` area-uniform samples
    (``ops.sample_mesh_surface`` with ``seed``), or with ``samples`` None the
    source's vertices.  A volume made from a mesh is observed only within its
    band, so no point counts as free there and hypotheses rank by inliers."""
    import torch

    from .. import ops
    from .tsdf_fusion import volume_from_mesh
    sv, sf = _mesh_arrays(src_mesh)
    dv, df = _mesh_arrays(dst_mesh)
    voxel = float(voxel)
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    dv_t, df_t = torch.as_tensor(dv).to(device), torch.as_tensor(df).to(device)
    fine = volume_from_mesh(dv_t, df_t, voxel, trunc)
    coarse = volume_from_mesh(dv_t, df_t, coarse_factor * voxel, coarse_factor * trunc)
    if samples is None:
        pts = torch.as_tensor(sv).to(device)
    else:
        sv_t, sf_t = torch.as_tensor(sv).to(device), torch.as_tensor(sf).to(device)
        ok = ((sf >= 0) & (sf < sv.shape[0])).all(1)
        tri = sv.astype(np.float64)[sf[ok]]
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        area = float(area[np.isfinite(area)].sum())
        if not area > 0.0:
            raise ValueError("global_register_meshes: the source mesh has no area")
        pts = ops.sample_mesh_surface(sv_t, sf_t, float(samples) / area, seed=int(seed))["points"]
    return global_register_points_tsdf(pts, fine, trunc, coarse=coarse,
                                       coarse_trunc=coarse_factor * trunc, device=device, **kw)
