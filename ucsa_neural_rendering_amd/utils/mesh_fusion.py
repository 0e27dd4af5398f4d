"""Per-frame 2D label maps fused onto a mesh by multi-view voting, on the GPU:
the mapping-based pseudo-label baseline (frame predictions -> 3D map -> frames)
out of the project's own parts.

    label maps --fuse_views--> vertex labels --ops.rasterize_mesh--> map_label

Every pixel of every view votes for the mesh vertex that the rasterizer gives it
(``ops.rasterize_mesh`` with ``vertex_labels = 1..V``: the nearest corner of the
hit point) with its frame's class; ``ops.fuse_label_votes`` sums the votes in a
uint64 table that stays on the device, ``ops.resolve_label_votes`` takes the
majority.  Hard votes only.  Out of scope: soft (probability-vector) votes,
filling unobserved vertices from their neighbours, voxel maps, registering a
mesh to the poses' frame (``load_mesh(..., pose_frame=True)`` covers the one
rigid motion the project records), anything in the training loop."""
from __future__ import annotations

import time

import numpy as np
import torch

from .. import ops


def _view(src, i):
    return src(i) if callable(src) else src[i]


def _batch(src, a, b, dtype, H, W, name):
    arr = np.stack([np.asarray(_view(src, i)) for i in range(a, b)])
    if arr.shape[1:] != (H, W):
        raise ValueError(f"{name}: views must be [{H},{W}], got {arr.shape[1:]}")
    return torch.from_numpy(np.ascontiguousarray(arr.astype(dtype, copy=False)))


def fuse_views(mesh, poses, intrinsics, H, W, near, label_maps, depth_maps=None,
               depth_tol=None, weights=None, num_classes=40, batch=16, min_votes=1,
               device="cuda"):
    """``mesh``: dict with verts [V,3] f32 and faces [F,3] int32 in the poses'
    (NGP) frame (``load_mesh``); ``poses`` [N,4,4]; ``label_maps``: a sequence
    or a callable ``i -> [H,W]`` integer class ids per view (NYU40: 1..C vote,
    everything else does not), read batch by batch; ``depth_maps`` likewise
    ``i -> [H,W]`` fp32 sensor z-depth in scene units (0 = none) with
    ``depth_tol``: a pixel then votes only where the mesh's z agrees with the
    sensor's within the tolerance; ``weights`` likewise ``i -> [H,W]`` integers
    in [0, 65535].  -> dict of numpy arrays ``labels`` [V] int32 (0 =
    unobserved or below ``min_votes``), ``total`` / ``winner`` [V] uint64,
    ``observed`` (count of labelled vertices), and the wall time split
    ``rasterize_ms`` / ``accumulate_ms`` (device-synchronised host clock)."""
    if (depth_maps is None) != (depth_tol is None):
        raise ValueError("depth_maps and depth_tol come as a pair")
    dev = torch.device(device)
    verts = torch.from_numpy(np.ascontiguousarray(mesh["verts"], np.float32)).to(dev)
    faces = torch.from_numpy(np.ascontiguousarray(mesh["faces"], np.int32)).to(dev)
    V = int(verts.shape[0])
    ids = torch.arange(1, V + 1, dtype=torch.int32, device=dev)
    votes = torch.zeros(V, int(num_classes) + 1, dtype=torch.int64, device=dev)
    poses = torch.as_tensor(np.asarray(poses, np.float32)).reshape(-1, 4, 4)
    t_r = t_a = 0.0
    for a in range(0, poses.shape[0], batch):
        b = min(a + batch, poses.shape[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ops.rasterize_mesh(verts, faces, poses[a:b].to(dev), intrinsics, H, W, near,
                                 vertex_labels=ids)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lab = _batch(label_maps, a, b, np.int64, H, W, "label_maps")
        # a class id outside uint8 cannot vote: map it to 0
        pred = torch.where((lab >= 0) & (lab <= 255), lab, torch.zeros_like(lab)) \
            .to(torch.uint8).to(dev)
        w = None if weights is None else \
            _batch(weights, a, b, np.int32, H, W, "weights").to(dev)
        sd = None if depth_maps is None else \
            _batch(depth_maps, a, b, np.float32, H, W, "depth_maps").to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ops.fuse_label_votes(votes, out["label"], pred, weight=w,
                             mesh_depth=None if sd is None else out["depth"],
                             sensor_depth=sd, depth_tol=depth_tol)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_r += t1 - t0
        t_a += t3 - t2
    res = ops.resolve_label_votes(votes, min_votes)
    labels = res["label"].cpu().numpy()
    return {"labels": labels,
            "total": res["total"].cpu().numpy().view(np.uint64),
            "winner": res["winner"].cpu().numpy().view(np.uint64),
            "observed": int((labels > 0).sum()),
            "rasterize_ms": 1e3 * t_r, "accumulate_ms": 1e3 * t_a}
