"""The voxel route of the mapping-based pseudo-label baseline, on the GPU: a
semantic voxel map instead of a labelled mesh.

    depth/ + poses + label maps --fuse_semantic_views--> volume, votes, labels
        --render_voxel_map--> map_label, map_depth
    depth/ + poses + score maps --fuse_semantic_views--> volume, evidence, labels

While ``ops.integrate_tsdf`` fuses a batch of depth views, ``ops.vote_voxel_labels``
lets the same views vote for their classes in the voxels of the truncation band;
``ops.resolve_voxel_labels`` keeps the winner per voxel and ``ops.raycast_tsdf``
ray-casts the volume into any posed view (depth, normal, the nearest voxel's
label).  No mesh is extracted and no per-view vertex-id render is needed.  With
``score_maps`` (rows of evidence codes per pixel, ``ops.log_evidence``) the
views add per-class evidence instead of one vote each
(``ops.accumulate_voxel_evidence`` / ``ops.resolve_voxel_evidence``): the label
of a voxel is then the MAP class of its views, not their majority.  With
``smooth`` the table is pooled over each observed voxel's observed neighbours
first (``ops.smooth_voxel_table``): a voxel that one view reached decides with
its neighbourhood, and a voxel that the geometry saw but no label reached takes
its neighbours' label.  Out of
scope: sparse / hashed blocks, float probabilities on the device, priors,
weights on the votes or the evidence (``view_weights`` weights the TSDF half
only), pose refinement."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .mesh_fusion import _batch, _score_batch
from .tsdf_fusion import depth_points_aabb, remove_small_components


def fuse_semantic_views(poses, intrinsics, H, W, depth_maps, label_maps, color_maps=None,
                        aabb=None, voxel=0.05, trunc=None, batch=16, num_classes=40,
                        min_votes=1, max_weight=65504.0, depth_min=1e-6, depth_max=3.0e38,
                        device="cuda", score_maps=None, min_margin=0, smooth=0,
                        smooth_neighbourhood=26, min_component=0, component_connectivity=26,
                        depth_filter=None, view_weights=None):
    """``poses`` [N,4,4] camera-to-world (NGP frame); ``depth_maps`` /
    ``label_maps`` / ``color_maps``: sequences or callables ``i -> [H,W]`` fp32
    z-depth in scene units (0 = none), ``[H,W]`` uint8 class ids (0 = no vote),
    ``[H,W,3]`` uint8 or None, read batch by batch.  The volume is picked as
    ``fuse_depth_views`` picks it (``aabb``, else the box of the back-projected
    depth points padded by ``trunc``; ``trunc`` defaults to 4 voxels).  -> dict:
    ``volume`` (``ops.tsdf_volume`` with ``trunc`` recorded), ``votes``
    [C+1,nx,ny,nz] uint16, ``labels`` [nx,ny,nz] uint8, ``total`` / ``winner``
    uint32, all on the device, and ``dims``, ``observed`` (share of voxels with
    weight >= 1), ``labelled`` (share with a label).
    With ``score_maps`` (``i -> [H,W,C]`` or ``[C,H,W]`` uint8 evidence codes,
    C = ``num_classes``; ``label_maps`` is then not read and may be None) the
    TSDF integration runs as before and the evidence path replaces the vote
    path: the dict carries ``evidence`` [C+1,nx,ny,nz] uint32 instead of
    ``votes``, ``labels`` resolved with ``min_votes`` as the least number of
    contributing views and ``min_margin`` as the least lead of the best class
    over the runner-up in evidence units, and ``views`` / ``best`` / ``margin``
    uint32 instead of ``total`` / ``winner``.
    ``smooth`` = N > 0 pools the table it built (votes or evidence) N times over
    each observed voxel's observed neighbours (``ops.smooth_voxel_table``,
    ``smooth_neighbourhood`` 6 or 26) before it is resolved; the dict then
    carries the pooled table, and ``min_votes`` / ``min_margin`` count pooled
    units (one pass over 26 neighbours multiplies a flat region's sums by up to
    27).  0 leaves everything as it was.
    ``min_component`` = N > 0 returns the components of the truncation band with
    fewer than N voxels to the unobserved state first
    (``tsdf_fusion.remove_small_components``, ``component_connectivity`` 6 or
    26), before the table is pooled and resolved and before any ray-cast: the
    floaters carry no label and no ray hits them; the dict then has their
    statistics as ``components``.  The table itself is not cleared: a removed
    voxel's column is never read again.
    ``depth_filter`` (a ``utils.depth_frontend.DepthFilter``) sends every frame
    through the depth front end first: the volume is integrated and the votes
    or the evidence are cast with the filtered frames without their rejected
    pixels, and the dict gains ``depth_filter``, the rejection counts.  None
    enters none of it.
    ``view_weights`` (a ``utils.depth_frontend.ViewWeights``; needs
    ``depth_filter``) integrates the TSDF half through
    ``ops.depth.integrate_tsdf_weighted`` with the confidence map of the same
    run of the front end; the integer vote and evidence tables are not
    weighted.  The volume's weight is then in units of pixel weight (a voxel seen
    once at w = 0.3 holds 0.3), which is what ``observed``, the ray-caster's and
    ``remove_small_components``' ``min_weight`` compare with; the dict gains
    ``view_weights``.  None enters none of it."""
    if view_weights is not None and depth_filter is None:
        raise ValueError("view_weights needs depth_filter: the weights come from that run's "
                         "points, normals and mask")
    df_stats = vw_stats = None
    if depth_filter is not None:
        from . import depth_frontend
        df_stats = depth_frontend.new_stats()
        if view_weights is not None:
            vw_stats = depth_frontend.new_weight_stats()
    smooth = int(smooth)
    if smooth < 0:
        raise ValueError("smooth must be >= 0")
    dev = torch.device(device)
    soft = score_maps is not None
    if not soft and min_margin:
        raise ValueError("min_margin applies to score_maps only")
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
    vol["trunc"] = trunc
    votes = ops.voxel_evidence(vol, num_classes) if soft else ops.voxel_votes(vol, num_classes)
    for a in range(0, N, batch):
        b = min(a + batch, N)
        z = _batch(depth_maps, a, b, np.float32, H, W, "depth_maps").to(dev)
        if soft:
            sc = _score_batch(score_maps, a, b, H, W, int(num_classes)).to(dev)
        else:
            lab = _batch(label_maps, a, b, np.uint8, H, W, "label_maps").to(dev)
        col = None
        if color_maps is not None:
            col = np.stack([np.asarray(color_maps(i) if callable(color_maps) else color_maps[i])
                            for i in range(a, b)])
            if col.shape[1:] != (H, W, 3):
                raise ValueError(f"color_maps: views must be [{H},{W},3], got {col.shape[1:]}")
            col = torch.from_numpy(np.ascontiguousarray(col.astype(np.uint8, copy=False))).to(dev)
        P = poses[a:b].to(dev)
        if view_weights is not None:
            z, pw = depth_frontend.weighted_depth(z, intrinsics, depth_filter, view_weights,
                                                  depth_min, depth_max, stats=df_stats,
                                                  weight_stats=vw_stats)
            ops.depth.integrate_tsdf_weighted(vol, z, pw, P, intrinsics, trunc, color=col,
                                              max_weight=max_weight, depth_min=depth_min,
                                              depth_max=depth_max)
        else:
            if depth_filter is not None:
                z = depth_frontend.clean_depth(z, intrinsics, depth_filter, depth_min,
                                               depth_max, stats=df_stats)
            ops.integrate_tsdf(vol, z, P, intrinsics, trunc, color=col, max_weight=max_weight,
                               depth_min=depth_min, depth_max=depth_max)
        if soft:
            ops.accumulate_voxel_evidence(votes, vol, z, sc, P, intrinsics, trunc,
                                          depth_min=depth_min, depth_max=depth_max)
        else:
            ops.vote_voxel_labels(votes, vol, z, lab, P, intrinsics, trunc, depth_min=depth_min,
                                  depth_max=depth_max)
    extra = {} if df_stats is None else {"depth_filter": df_stats}
    if vw_stats is not None:
        extra["view_weights"] = vw_stats
    if int(min_component) > 0:
        extra["components"] = remove_small_components(vol, int(min_component),
                                                      component_connectivity)
    if smooth:
        votes = ops.smooth_voxel_table(votes, vol, neighbourhood=smooth_neighbourhood,
                                       iterations=smooth)
    if soft:
        res = ops.resolve_voxel_evidence(votes, min_votes, min_margin)
        return {**extra, "volume": vol, "evidence": votes, "labels": res["label"], "views": res["views"],
                "best": res["best"], "margin": res["margin"], "dims": tuple(dims),
                "observed": float((vol["weight"] >= 1.0).float().mean()),
                "labelled": float((res["label"] > 0).float().mean())}
    res = ops.resolve_voxel_labels(votes, min_votes)
    return {**extra, "volume": vol, "votes": votes, "labels": res["label"], "total": res["total"],
            "winner": res["winner"], "dims": tuple(dims),
            "observed": float((vol["weight"] >= 1.0).float().mean()),
            "labelled": float((res["label"] > 0).float().mean())}


def render_voxel_map(volume, voxel_labels, poses, intrinsics, H, W, near, far, step=None,
                     min_weight=1.0, batch=16):
    """Yields (first view index, ``ops.raycast_tsdf`` dict of device tensors) for
    the views in batches of ``batch``."""
    dev = volume["tsdf"].device
    poses = torch.as_tensor(np.asarray(poses, np.float32)).reshape(-1, 4, 4)
    for a in range(0, poses.shape[0], batch):
        yield a, ops.raycast_tsdf(volume, poses[a:a + batch].to(dev), intrinsics, H, W, near,
                                  far, step=step, min_weight=min_weight,
                                  voxel_labels=voxel_labels)
