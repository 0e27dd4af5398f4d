"""A scene's mesh from its posed depth frames, on the GPU: projective TSDF
fusion into a dense volume, then marching cubes over the observed cells.  The
first stage of the mapping-based pseudo-label baseline, so that the chain runs
from a scene directory alone:

    depth/ + poses --fuse_depth_views--> mesh --mesh_fusion.fuse_views--> labels
        --ops.rasterize_mesh--> map_label

``ops.integrate_tsdf`` updates the volume with a batch of views per call (the
voxel state is read and written once per batch); ``ops.marching_cubes`` with
``valid = weight >= min_weight`` meshes ``-tsdf`` at 0 and leaves out every cell
with an unobserved corner (no second sheet one truncation distance behind the
walls).  Per-voxel class votes and the ray-cast model view of the volume are in
``utils/voxel_map.py``.  Out of scope: sparse / hashed voxel blocks, bilinear
depth lookup, anything in the training loop.  ``view_weights`` (with
``depth_filter``) integrates every pixel with a weight from its range and
viewing angle (``ops.depth.integrate_tsdf_weighted``).  ``fuse_depth_views(refine_poses=True)`` refines each frame's pose against
the volume before it is integrated (``track_depth_views``).

``remove_small_components`` drops the floaters first: the specks of truncation
band that a few bad depth pixels leave in observed free space.  The band
(``band_mask``) is labelled by ``ops.voxel_components``, sized by
``ops.component_sizes``, and every component below a voxel count goes back to
the volume's empty state, so that neither the mesh nor the ray-caster sees it."""
from __future__ import annotations

import time

import numpy as np
import torch

from .. import ops
from .mesh_fusion import _batch


def depth_points_aabb(poses, intrinsics, depth_maps, H, W, batch=16, depth_min=1e-6,
                      depth_max=3.0e38, device="cuda"):
    """Bounding box [2,3] (numpy f32, poses' frame) of the back-projected valid
    depth points of all views, computed on the device batch by batch."""
    dev = torch.device(device)
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    poses = torch.as_tensor(np.asarray(poses, np.float32)).reshape(-1, 4, 4)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, torch.ones_like(xs)], -1)
    lo = torch.full((3,), float("inf"), device=dev)
    hi = torch.full((3,), float("-inf"), device=dev)
    for a in range(0, poses.shape[0], batch):
        b = min(a + batch, poses.shape[0])
        z = _batch(depth_maps, a, b, np.float32, H, W, "depth_maps").to(dev)
        P = poses[a:b].to(dev)
        ok = torch.isfinite(z) & (z >= depth_min) & (z <= depth_max)
        pc = ray[None] * torch.where(ok, z, torch.zeros_like(z))[..., None]
        pw = torch.einsum("bhwc,brc->bhwr", pc, P[:, :3, :3]) + P[:, None, None, :3, 3]
        inf = torch.full_like(pw, float("inf"))
        lo = torch.minimum(lo, torch.where(ok[..., None], pw, inf).amin((0, 1, 2)))
        hi = torch.maximum(hi, torch.where(ok[..., None], pw, -inf).amax((0, 1, 2)))
    if not bool(torch.isfinite(lo).all() and torch.isfinite(hi).all()):
        raise ValueError("no valid depth measurement in any view")
    return torch.stack([lo, hi]).cpu().numpy()


def extract_mesh(volume, min_weight=1):
    """A volume of ``ops.tsdf_volume`` -> (verts, faces, normals, rgb or None)
    on the device: ``-tsdf`` at iso 0 over the cells whose corners all have
    weight >= min_weight; a vertex takes the colour of the nearer end point of
    its edge (both are observed)."""
    valid = volume["weight"] >= float(min_weight)
    verts, faces, normals = ops.marching_cubes(-volume["tsdf"], 0.0, volume["origin"],
                                               volume["spacing"], valid=valid)
    rgb = None
    if volume.get("rgb") is not None:
        dev = verts.device
        o = torch.tensor(volume["origin"], device=dev)
        h = torch.tensor(volume["spacing"], device=dev)
        top = torch.tensor(volume["tsdf"].shape, device=dev) - 1
        q = torch.minimum(torch.round((verts - o) / h).long().clamp_(min=0), top)
        rgb = (volume["rgb"][q[:, 0], q[:, 1], q[:, 2]] / 255.0).clamp_(0.0, 1.0)
    return verts, faces, normals, rgb


def band_mask(volume, min_weight=1):
    """bool [nx,ny,nz]: the observed voxels that are not free space,
    ``(weight >= min_weight) & (tsdf < 1)``.  A NaN weight is not observed, as
    everywhere else."""
    return (volume["weight"] >= float(min_weight)) & (volume["tsdf"] < 1.0)


def component_stats(sizes, is_root, min_size):
    """``sizes`` int32 (``ops.component_sizes``), ``is_root`` bool of the same
    shape (one element per component) -> the statistics dict; the elements of
    the components below ``min_size`` count as removed."""
    root_sizes = sizes[is_root]
    small = root_sizes < int(min_size)
    return {"components": int(root_sizes.numel()), "removed_components": int(small.sum()),
            "removed": int(root_sizes[small].sum()),
            "largest": int(root_sizes.max()) if root_sizes.numel() else 0}


def remove_small_components(volume, min_voxels, connectivity=26, min_weight=1):
    """Return every voxel of ``band_mask(volume, min_weight)`` whose component
    (``connectivity`` 6 or 26) has fewer than ``min_voxels`` voxels to
    ``ops.tsdf_volume``'s empty state, in place: tsdf 1, weight 0, rgb 0.  The
    cleared voxels are unobserved again: ``marching_cubes(valid=)`` and
    ``raycast_tsdf`` ignore them and a later ``integrate_tsdf`` restarts them
    clean.  -> {"components": n, "removed_components": m, "removed_voxels": k,
    "largest": s}.  ``min_voxels`` <= 1 touches nothing.  The labelling and the
    counts are the kernels'; the clear is torch indexing."""
    band = band_mask(volume, min_weight)
    labels = ops.voxel_components(band, connectivity)
    sizes = ops.component_sizes(labels)
    n = labels.numel()
    is_root = labels.view(-1) == torch.arange(n, dtype=torch.int32, device=labels.device)
    st = component_stats(sizes.view(-1), is_root, min_voxels)
    out = {"components": st["components"], "removed_components": st["removed_components"],
           "removed_voxels": st["removed"], "largest": st["largest"]}
    if int(min_voxels) > 1 and out["removed_voxels"]:
        drop = band & (sizes < int(min_voxels))
        volume["tsdf"][drop] = 1.0
        volume["weight"][drop] = 0.0
        if volume.get("rgb") is not None:
            volume["rgb"][drop] = 0.0
    return out


def fuse_depth_views(poses, intrinsics, H, W, depth_maps, color_maps=None, aabb=None,
                     voxel=0.05, trunc=None, min_weight=1, batch=16, max_weight=65504.0,
                     depth_min=1e-6, depth_max=3.0e38, device="cuda", min_component=0,
                     component_connectivity=26, refine_poses=False, refine_warmup=1,
                     refine_kw=None, refine_min_matched=0.25, refine_max_step=None,
                     depth_filter=None, view_weights=None, refine_method="tsdf"):
    """``poses`` [N,4,4] camera-to-world (NGP frame); ``depth_maps``: a sequence
    or a callable ``i -> [H,W]`` fp32 z-depth in scene units (0 = none), read
    batch by batch; ``color_maps`` likewise ``i -> [H,W,3]`` uint8 or None;
    ``aabb`` [2,3] or 6 numbers (lo, hi) of the volume, None = the bounding box
    of the back-projected valid depth points padded by ``trunc``; ``voxel`` the
    lattice spacing and ``trunc`` the truncation distance in scene units
    (default: 4 voxels).  -> a mesh dict as ``load_mesh`` gives it (numpy, NGP
    frame): verts [V,3] f32, faces [F,3] int32, normals [V,3] f32, rgb [V,3]
    f32 in [0,1] or None, labels None; plus ``dims``, ``origin``, ``spacing``,
    ``observed`` (share of voxels with weight >= min_weight) and the wall-time
    split ``integrate_ms`` / ``extract_ms`` (device-synchronised host clock).
    ``min_component`` > 0 runs ``remove_small_components`` with that voxel count
    (and ``component_connectivity``) before the mesh is extracted and adds its
    statistics as ``components``.  ``refine_poses`` tracks the camera against the
    model while it is fused (``track_depth_views``, which the ``refine_*``
    arguments go to): the box is still computed from the given poses, the views
    are integrated one per call, and the dict gains ``poses`` [N,4,4] float64
    (the poses used), ``refine`` (the per-frame records) and ``refine_ms``.
    ``refine_method`` "tsdf" (the default) or "projective" chooses the tracker, as
    in ``track_depth_views``.
    With ``refine_poses=False`` nothing of that is entered and every byte of the
    result is what it was.  ``depth_filter`` (a ``utils.depth_frontend.DepthFilter``)
    sends every frame through the depth front end first: the volume is
    integrated with the filtered frames without their rejected pixels, tracking
    takes the kept pixels' points, and the dict gains ``depth_filter``, the
    rejection counts (``depth_frontend.stats_line`` prints them).  The box is
    still that of the raw frames.  None enters none of it.  ``view_weights`` (a
    ``utils.depth_frontend.ViewWeights``; needs ``depth_filter``, whose points,
    normals and mask it reads) integrates the cleaned frames through
    ``ops.depth.integrate_tsdf_weighted`` with ``depth_confidence``'s map, and
    the dict gains ``view_weights`` (``depth_frontend.weight_stats_line``).  The
    volume's weight, and so ``min_weight``, is then in units of pixel weight: a
    voxel seen once at w = 0.3 holds 0.3, and ``min_weight`` =
    ``view_weights.least(depth_filter, z_max)`` keeps what 1 keeps without
    weights.  None enters none of it."""
    dev = torch.device(device)
    if view_weights is not None and depth_filter is None:
        raise ValueError("view_weights needs depth_filter: the weights come from that run's "
                         "points, normals and mask")
    df_stats = vw_stats = None
    if depth_filter is not None:
        from . import depth_frontend
        df_stats = depth_frontend.new_stats()
        if view_weights is not None:
            vw_stats = depth_frontend.new_weight_stats()
    voxel = float(voxel)
    trunc = 4.0 * voxel if trunc is None else float(trunc)
    if not (voxel > 0 and trunc > 0):
        raise ValueError("voxel and trunc must be > 0")
    poses = torch.as_tensor(np.asarray(poses, np.float32)).reshape(-1, 4, 4)
    N = int(poses.shape[0])
    if N == 0:
        raise ValueError("no views")
    if aabb is None:
        box = depth_points_aabb(poses, intrinsics, depth_maps, H, W, batch, depth_min,
                                depth_max, dev)
        box = box + np.array([[-trunc], [trunc]], np.float32)
    else:
        box = np.asarray(aabb, np.float32).reshape(2, 3)
    dims = [max(2, int(np.ceil(float(box[1, a] - box[0, a]) / voxel - 1e-6)) + 1)
            for a in range(3)]
    vol = ops.tsdf_volume(dims, box[0].tolist(), voxel, with_color=color_maps is not None,
                          device=dev)
    t_i = 0.0
    tracked = None
    if refine_poses:
        tracked = track_depth_views(vol, poses, intrinsics, H, W, depth_maps, trunc,
                                    color_maps=color_maps, min_weight=min_weight,
                                    max_weight=max_weight, depth_min=depth_min,
                                    depth_max=depth_max, refine_warmup=refine_warmup,
                                    refine_kw=refine_kw, refine_min_matched=refine_min_matched,
                                    refine_max_step=refine_max_step,
                                    **({} if refine_method == "tsdf" else
                                       {"refine_method": refine_method}),
                                    **({} if depth_filter is None else
                                       {"depth_filter": depth_filter, "depth_filter_stats": df_stats}),
                                    **({} if view_weights is None else
                                       {"view_weights": view_weights, "view_weight_stats": vw_stats}))
        t_i = 1e-3 * tracked["integrate_ms"]
    # tracked: every view is in the volume already; otherwise a batch of views per call
    for a in ([] if tracked is not None else range(0, N, batch)):
        b = min(a + batch, N)
        z = _batch(depth_maps, a, b, np.float32, H, W, "depth_maps").to(dev)
        col = None
        if color_maps is not None:
            col = np.stack([np.asarray(color_maps(i) if callable(color_maps) else color_maps[i])
                            for i in range(a, b)])
            if col.shape[1:] != (H, W, 3):
                raise ValueError(f"color_maps: views must be [{H},{W},3], got {col.shape[1:]}")
            col = torch.from_numpy(np.ascontiguousarray(col.astype(np.uint8, copy=False))).to(dev)
        P = poses[a:b].to(dev)
        pw = None
        if view_weights is not None:
            z, pw = depth_frontend.weighted_depth(z, intrinsics, depth_filter, view_weights,
                                                  depth_min, depth_max, stats=df_stats,
                                                  weight_stats=vw_stats)
        elif depth_filter is not None:
            z = depth_frontend.clean_depth(z, intrinsics, depth_filter, depth_min, depth_max,
                                           stats=df_stats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if pw is not None:
            ops.depth.integrate_tsdf_weighted(vol, z, pw, P, intrinsics, trunc, color=col,
                                              max_weight=max_weight, depth_min=depth_min,
                                              depth_max=depth_max)
        else:
            ops.integrate_tsdf(vol, z, P, intrinsics, trunc, color=col, max_weight=max_weight,
                               depth_min=depth_min, depth_max=depth_max)
        torch.cuda.synchronize()
        t_i += time.perf_counter() - t0
    stats = None
    if int(min_component) > 0:
        stats = remove_small_components(vol, int(min_component), component_connectivity,
                                        min_weight)
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    verts, faces, normals, rgb = extract_mesh(vol, min_weight)
    torch.cuda.synchronize()
    t_e = time.perf_counter() - t0
    observed = float((vol["weight"] >= float(min_weight)).float().mean())
    extra = {} if stats is None else {"components": stats}
    if tracked is not None:
        extra.update(poses=tracked["poses"], refine=tracked["refine"],
                     refine_ms=tracked["refine_ms"])
    if df_stats is not None:
        extra["depth_filter"] = df_stats
    if vw_stats is not None:
        extra["view_weights"] = vw_stats
    return {**extra, "verts": verts.cpu().numpy(), "faces": faces.cpu().numpy(),
            "normals": normals.cpu().numpy(),
            "rgb": None if rgb is None else rgb.cpu().numpy(), "labels": None,
            "dims": tuple(dims), "origin": vol["origin"], "spacing": vol["spacing"],
            "observed": observed, "integrate_ms": 1e3 * t_i, "extract_ms": 1e3 * t_e}


def track_depth_views(volume, poses, intrinsics, H, W, depth_maps, trunc, color_maps=None,
                      min_weight=1, max_weight=65504.0, depth_min=1e-6, depth_max=3.0e38,
                      refine_warmup=1, refine_kw=None, refine_min_matched=0.25,
                      refine_max_step=None, depth_filter=None, depth_filter_stats=None,
                      view_weights=None, view_weight_stats=None, refine_method="tsdf"):
    """Frame-to-model tracking, the other half of KinectFusion: integrate the
    views into ``volume`` (in place) one per call, each with a pose refined
    against the volume as it then stands.  The first ``refine_warmup`` frames
    are integrated with their given poses; each later frame goes through
    ``utils.registration.refine_pose_tsdf`` with ``init`` = its given pose
    (``refine_kw``: its keyword arguments, ``stride``, ``iterations``,
    ``max_tsdf_schedule`` ...; ``min_weight`` defaults to this call's) and is
    integrated with the refined pose.  A frame keeps its given pose and counts
    as a fallback when the last solve's rank is below 6, when the matched share
    of its back-projected points is below ``refine_min_matched``, or when the
    refined pose differs from the given one by more than ``refine_max_step`` =
    (radians, units), default (0.1, ``trunc``): a larger step has left the basin
    in which the volume carries signal.  -> dict: ``poses`` [N,4,4] float64 (the
    poses used), ``refine`` (per frame None during the warm-up, else a dict
    ``matched`` -- the share --, ``rmse``, ``rank``, ``iterations``, ``step``
    (radians, units) from the given pose and ``fallback``), ``integrate_ms``,
    ``refine_ms`` (device-synchronised host clock).  With ``depth_filter`` (a
    ``utils.depth_frontend.DepthFilter``) a frame is tracked with the points of
    the pixels the front end keeps and integrated with its cleaned depth;
    ``depth_filter_stats`` (``depth_frontend.new_stats()``) gains the counts of
    the integrated frames.  ``view_weights`` (a ``ViewWeights``; needs
    ``depth_filter``) integrates each frame through
    ``ops.depth.integrate_tsdf_weighted`` with the confidence map of the same
    run of the front end; the volume's weight is then in units of pixel weight,
    and so is the ``min_weight`` tracking compares it with.
    ``view_weight_stats`` (``depth_frontend.new_weight_stats()``) gains the kept
    pixels' count and weight.  ``refine_method`` "projective" tracks with
    ``utils.registration.refine_pose_projective`` instead -- the model ray-cast
    from the given pose, projective association, the gate ``max_dist`` in place
    of the truncation band -- under the same fallback rules; ``refine_kw`` is
    then its keyword arguments (an integer ``iterations`` means one level; a
    ``stride`` other than 1 is an error: the pyramid is its way to fewer
    points)."""
    from .registration import pose_step, refine_pose_projective, refine_pose_tsdf
    if refine_method not in ("tsdf", "projective"):
        raise ValueError(f"refine_method must be 'tsdf' or 'projective', got {refine_method!r}")
    if view_weights is not None and depth_filter is None:
        raise ValueError("view_weights needs depth_filter: the weights come from that run's "
                         "points, normals and mask")
    if depth_filter is not None:
        from . import depth_frontend
        kw_filter = {"depth_filter": depth_filter}
    else:
        kw_filter = {}
    dev = volume["tsdf"].device
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    kw = dict(refine_kw or {})
    kw.setdefault("min_weight", float(min_weight))
    if refine_method == "projective":
        if int(kw.pop("stride", 1)) != 1:
            raise ValueError("refine_method='projective' takes no stride")
        if isinstance(kw.get("iterations"), int):
            kw["iterations"] = (kw["iterations"],)
    max_rot, max_trans = (0.1, float(trunc)) if refine_max_step is None else refine_max_step
    used, records, t_i, t_r = [], [], 0.0, 0.0
    for i in range(poses.shape[0]):
        z = _batch(depth_maps, i, i + 1, np.float32, H, W, "depth_maps").to(dev)
        col = None
        if color_maps is not None:
            col = np.asarray(color_maps(i) if callable(color_maps) else color_maps[i])
            if col.shape != (H, W, 3):
                raise ValueError(f"color_maps: views must be [{H},{W},3], got {col.shape}")
            col = torch.from_numpy(np.ascontiguousarray(col.astype(np.uint8, copy=False))[None])
            col = col.to(dev)
        given = poses[i].astype(np.float64)
        pose, rec = given, None
        if i >= int(refine_warmup):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if refine_method == "projective":
                out = refine_pose_projective(z[0], given, intrinsics, volume, trunc,
                                             depth_min=depth_min, depth_max=depth_max,
                                             **kw_filter, **kw)
            else:
                out = refine_pose_tsdf(z[0], given, intrinsics, volume, trunc,
                                       depth_min=depth_min, depth_max=depth_max, device=dev,
                                       **kw_filter, **kw)
            t_r += time.perf_counter() - t0
            rot, trans = pose_step(out["pose"], given)
            share = out["matched"] / out["n_points"] if out["n_points"] else 0.0
            fallback = bool(out["rank"] < 6 or share < refine_min_matched or rot > max_rot
                            or trans > max_trans)
            rec = {"matched": share, "rmse": out["rmse"], "rank": out["rank"],
                   "iterations": out["iterations"], "step": (rot, trans), "fallback": fallback}
            if not fallback:
                pose = out["pose"]
        used.append(pose)
        records.append(rec)
        P = torch.from_numpy(pose.astype(np.float32)[None]).to(dev)
        pw = None
        if view_weights is not None:
            z, pw = depth_frontend.weighted_depth(z, intrinsics, depth_filter, view_weights,
                                                  depth_min, depth_max, stats=depth_filter_stats,
                                                  weight_stats=view_weight_stats)
        elif depth_filter is not None:
            z = depth_frontend.clean_depth(z, intrinsics, depth_filter, depth_min, depth_max,
                                           stats=depth_filter_stats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if pw is not None:
            ops.depth.integrate_tsdf_weighted(volume, z, pw, P, intrinsics, trunc, color=col,
                                              max_weight=max_weight, depth_min=depth_min,
                                              depth_max=depth_max)
        else:
            ops.integrate_tsdf(volume, z, P, intrinsics, trunc, color=col, max_weight=max_weight,
                               depth_min=depth_min, depth_max=depth_max)
        torch.cuda.synchronize()
        t_i += time.perf_counter() - t0
    return {"poses": np.stack(used), "refine": records, "integrate_ms": 1e3 * t_i,
            "refine_ms": 1e3 * t_r}


def volume_from_mesh(verts, faces, voxel, trunc, aabb=None, max_voxels=1 << 28):
    """A TSDF volume made from a triangle mesh instead of from depth frames
    (``ops.mesh_tsdf``): a ground-truth mesh, an earlier stage's export or a
    simplified mesh can then be ray-cast (``ops.raycast_tsdf``), re-meshed at a
    uniform step (``extract_mesh``), turned into the occupancy prior
    (``ops.tsdf_occupancy``) or compared voxel by voxel with a fused volume
    (``utils.mesh_eval.tsdf_bias``).  The lattice is ``voxel_iou``'s rule padded
    by ``trunc``: cubic with spacing ``voxel`` over the box of the finite
    vertices (or ``aabb`` [2,3]), origin = lo - (trunc + voxel), dims =
    ceil((hi + (trunc + voxel) - origin) / voxel) + 1 per axis, in float32.
    Voxels within ``trunc`` of the surface hold tsdf = clamp(sdf / trunc, -1, 1)
    and weight 1, all others tsdf 1 and weight 0 (free, unobserved), as after
    ``ops.integrate_tsdf``; positive is the side the faces' (B-A)x(C-A) points
    to, so the mesh must be counter-clockwise seen from free space
    (``ops.marching_cubes`` of ``-tsdf``, which ``extract_mesh`` uses, makes
    such meshes).  More than ``max_voxels`` voxels is an error raised before
    anything of that size is allocated."""
    v = torch.as_tensor(np.asarray(verts, np.float32) if not torch.is_tensor(verts) else verts)
    v = v.to(device="cuda" if not v.is_cuda else v.device, dtype=torch.float32).reshape(-1, 3)
    v = v.contiguous()
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces)
    f = f.to(device=v.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    voxel, trunc = float(np.float32(voxel)), float(np.float32(trunc))
    if not (voxel > 0 and np.isfinite(voxel) and trunc > 0 and np.isfinite(trunc)):
        raise ValueError(f"voxel and trunc must be > 0 and finite, got {voxel}, {trunc}")
    if aabb is None:
        pts = v[torch.isfinite(v).all(1)]
        if pts.shape[0] == 0:
            raise ValueError("volume_from_mesh: no finite vertex and no aabb")
        box = torch.stack([pts.amin(0), pts.amax(0)]).cpu().numpy()
    else:
        box = np.asarray(aabb, np.float32).reshape(2, 3)
    pad = np.float32(trunc) + np.float32(voxel)
    lo = (box[0] - pad).astype(np.float32)
    hi = (box[1] + pad).astype(np.float32)
    dims = tuple(int(np.ceil(float(hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    if dims[0] * dims[1] * dims[2] > min(int(max_voxels), 0x7FFFFFFF):
        raise ValueError(f"voxel {voxel} gives {dims} voxels, more than max_voxels = "
                         f"{max_voxels}: raise voxel")
    volume = ops.tsdf_volume(dims, [float(x) for x in lo], voxel, device=v.device)
    return ops.mesh_tsdf(volume, v, f, trunc)
