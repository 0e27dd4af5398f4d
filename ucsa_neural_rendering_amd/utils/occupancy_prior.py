"""An occupancy prior for the marcher from the scene's own depth frames: the
mapping chain already knows which space the sensor saw to be empty, in the
NeRF's frame, so the marcher need not learn it.

    depth/ + poses --ops.integrate_tsdf--> volume --ops.tsdf_occupancy--> mask
        --SemanticNeRFRenderer.set_occupancy_prior--> density_grid = -1 there

A fresh field has sigma ~ 1 everywhere and the marcher walks the air densely
until the grid has forgotten it (``refresh_due``); with the prior the measured
free space is skipped from step 0 and stays skipped.  The volume is picked the
way ``tsdf_fusion.fuse_depth_views`` picks it.

A scene that comes with a mesh (ScanNet's ``*_vh_clean_2.ply``, the PLY of an
earlier ``fuse_tsdf_mesh.py`` run, the previous stage's exported field) needs no
depth frames and no volume: ``prior_from_mesh`` keeps the shell of cells the
mesh passes through (``ops.mesh_occupancy``).

    mesh --ops.mesh_occupancy--> mask --set_occupancy_prior--> density_grid

Out of scope: carving straight from depth views without a volume,
camera-coverage marking without depth, sparse volumes."""
from __future__ import annotations

import time

import numpy as np
import torch

from .. import ops
from .mesh_fusion import _batch
from .tsdf_fusion import depth_points_aabb


def volume_from_depth_views(poses, intrinsics, H, W, depth_maps, voxel=0.05, trunc=None,
                            aabb=None, batch=16, max_weight=65504.0, depth_min=1e-6,
                            depth_max=3.0e38, device="cuda", depth_filter=None,
                            depth_filter_stats=None, view_weights=None,
                            view_weight_stats=None):
    """The TSDF volume (``ops.tsdf_volume``, no colour) of the views, chosen and
    integrated as ``fuse_depth_views`` does -> (volume, trunc, integrate_ms).
    ``depth_filter`` / ``depth_filter_stats`` and ``view_weights`` /
    ``view_weight_stats`` as for ``track_depth_views``."""
    if view_weights is not None and depth_filter is None:
        raise ValueError("view_weights needs depth_filter: the weights come from that run's "
                         "points, normals and mask")
    if depth_filter is not None:
        from . import depth_frontend
    dev = torch.device(device)
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
    vol = ops.tsdf_volume(dims, box[0].tolist(), voxel, device=dev)
    t_i = 0.0
    for a in range(0, N, batch):
        b = min(a + batch, N)
        z = _batch(depth_maps, a, b, np.float32, H, W, "depth_maps").to(dev)
        P = poses[a:b].to(dev)
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
            ops.depth.integrate_tsdf_weighted(vol, z, pw, P, intrinsics, trunc,
                                              max_weight=max_weight, depth_min=depth_min,
                                              depth_max=depth_max)
        else:
            ops.integrate_tsdf(vol, z, P, intrinsics, trunc, max_weight=max_weight,
                               depth_min=depth_min, depth_max=depth_max)
        torch.cuda.synchronize()
        t_i += time.perf_counter() - t0
    return vol, trunc, 1e3 * t_i


def prior_from_depth_views(poses, intrinsics, H, W, depth_maps, bound, voxel=0.05, trunc=None,
                           aabb=None, batch=16, depth_filter=None, view_weights=None,
                           **occupancy_kw):
    """``poses`` [N,4,4] camera-to-world (NGP frame), ``depth_maps`` a sequence
    or callable ``i -> [H,W]`` fp32 z-depth in scene units (0 = none), ``bound``
    the renderer's; ``voxel`` / ``trunc`` (default 4 voxels) / ``aabb`` (None =
    the box of the valid depth points padded by ``trunc``) as for
    ``fuse_depth_views``; ``occupancy_kw`` goes to ``ops.tsdf_occupancy``
    (cascade, H, dilate, min_weight, free_tsdf, unknown).  -> (mask uint8
    [cascade,H,H,H] on the device, stats): ``kept`` the kept share per cascade,
    ``observed`` / ``band`` / ``free`` the shares of the volume's voxels with
    weight >= min_weight / observed and not free / observed and free, ``dims``,
    ``origin``, ``spacing``, ``trunc`` and the wall time ``integrate_ms`` /
    ``occupancy_ms`` (device-synchronised host clock).  ``depth_filter`` (a
    ``utils.depth_frontend.DepthFilter``) integrates the frames as the depth
    front end cleans them and adds the rejection counts to the stats as
    ``depth_filter``; None enters none of it.  ``view_weights`` (a
    ``utils.depth_frontend.ViewWeights``; needs ``depth_filter``) integrates them
    through ``ops.depth.integrate_tsdf_weighted`` with the confidence map of the
    same run and adds ``view_weights`` to the stats.  The volume's weight is then
    in units of pixel weight -- a voxel seen once at w = 0.3 holds 0.3 -- and so is
    ``min_weight``: ``view_weights.least(depth_filter, z_max)`` carves what 1
    carves without weights, the default of 1 only what several good views agree
    on.  None enters none of it."""
    if view_weights is not None and depth_filter is None:
        raise ValueError("view_weights needs depth_filter: the weights come from that run's "
                         "points, normals and mask")
    df_kw = {}
    if depth_filter is not None:
        from . import depth_frontend
        df_kw = {"depth_filter": depth_filter, "depth_filter_stats": depth_frontend.new_stats()}
    if view_weights is not None:
        df_kw.update(view_weights=view_weights,
                     view_weight_stats=depth_frontend.new_weight_stats())
    vol, trunc, t_i = volume_from_depth_views(poses, intrinsics, H, W, depth_maps, voxel, trunc,
                                              aabb, batch, **df_kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mask = ops.tsdf_occupancy(vol, bound, **occupancy_kw)
    torch.cuda.synchronize()
    t_o = time.perf_counter() - t0
    seen = vol["weight"] >= float(occupancy_kw.get("min_weight", 1.0))
    free = seen & (vol["tsdf"] >= float(occupancy_kw.get("free_tsdf", 1.0)))
    stats = {"kept": [float(v) for v in mask.float().mean((1, 2, 3)).tolist()],
             "observed": float(seen.float().mean()), "band": float((seen & ~free).float().mean()),
             "free": float(free.float().mean()), "dims": tuple(vol["tsdf"].shape),
             "origin": vol["origin"], "spacing": vol["spacing"], "trunc": trunc,
             "integrate_ms": t_i, "occupancy_ms": 1e3 * t_o}
    if depth_filter is not None:
        stats["depth_filter"] = df_kw["depth_filter_stats"]
    if view_weights is not None:
        stats["view_weights"] = df_kw["view_weight_stats"]
    return mask, stats


def prior_from_mesh(verts, faces, bound, **mesh_occupancy_kw):
    """``verts`` [V,3] / ``faces`` [F,3] (numpy or tensors) in the field's (NGP)
    frame, ``bound`` the renderer's; ``mesh_occupancy_kw`` goes to
    ``ops.mesh_occupancy`` (cascade, H, dilate).  -> (mask uint8 [cascade,H,H,H]
    on the device, stats): ``kept`` the kept share per cascade, ``faces`` the
    face count, ``skipped`` the faces that mark nothing because a corner is not
    finite, ``dilate`` as used, and the wall time ``voxelize_ms``
    (device-synchronised host clock)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    v = torch.as_tensor(np.asarray(verts, np.float32) if not torch.is_tensor(verts) else verts)
    v = v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces)
    f = f.to(device=dev, dtype=torch.int32).reshape(-1, 3).contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mask = ops.mesh_occupancy(v, f, bound, **mesh_occupancy_kw)
    torch.cuda.synchronize()
    t_v = time.perf_counter() - t0
    skipped = int((~torch.isfinite(v)[f.long()].all(-1).all(-1)).sum()) if f.shape[0] else 0
    dilate = mesh_occupancy_kw.get("dilate")
    if dilate is None:
        dilate = 2.0 * min(1.0, float(bound)) / int(mask.shape[1])
    stats = {"kept": [float(x) for x in mask.float().mean((1, 2, 3)).tolist()],
             "faces": int(f.shape[0]), "skipped": skipped, "dilate": float(dilate),
             "voxelize_ms": 1e3 * t_v}
    return mask, stats


def save_prior(path, mask, bound, **params):
    """Write the mask (bit-packed: 128^3 x 3 cascades is 768 KiB) and its
    parameters as an ``.npz`` that ``load_prior`` reads."""
    m = np.ascontiguousarray(torch.as_tensor(mask).cpu().numpy() != 0)
    extra = {k: np.asarray(v) for k, v in params.items() if v is not None}
    np.savez_compressed(path, mask_bits=np.packbits(m.reshape(-1)),
                        shape=np.asarray(m.shape, np.int64), bound=np.float32(bound), **extra)


def load_prior(path):
    """-> (mask uint8 [cascade,H,H,H] numpy, params dict) of ``save_prior``"""
    with np.load(path) as z:
        shape = tuple(int(v) for v in z["shape"])
        n = int(np.prod(shape))
        mask = np.unpackbits(z["mask_bits"])[:n].reshape(shape).astype(np.uint8)
        params = {k: z[k] for k in z.files if k not in ("mask_bits", "shape")}
    return mask, params
