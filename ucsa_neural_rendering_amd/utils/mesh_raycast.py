"""Ray casts against a mesh for whole views and for visibility
(``ops.raycast.raycast_mesh`` / ``ops.raycast.mesh_occluded`` over
``ops.triangle_grid``).

``raycast_views`` gives what ``ops.rasterize_mesh`` gives -- face, z-depth, label
and colour per pixel -- from one exact ray per pixel centre instead of from
snapped vertices; it is slower than the rasterizer for whole views and is meant
for comparison and for rays the rasterizer cannot serve.

``visible_points`` counts, per point, the views that see it: inside the image,
inside the depth range, and with a free segment from the camera centre.  The 3D
scores use it to leave out ground-truth surface that no camera observed
(``utils.mesh_eval``: ``visible_from``)."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops


def _dev_mesh(mesh, device):
    dev = torch.device(device)
    verts = torch.as_tensor(np.asarray(mesh["verts"], np.float32)).to(dev).reshape(-1, 3)
    faces = torch.as_tensor(np.asarray(mesh["faces"], np.int32)).to(dev).reshape(-1, 3)
    return verts.contiguous(), faces.contiguous()


def raycast_views(mesh, poses, intrinsics, H, W, near, far, batch=16, device="cuda", grid=None,
                  sort_rays=False):
    """The mesh (``load_mesh``'s dict) seen from ``poses`` [B,4,4] by one ray per
    pixel centre (``ops.get_rays``) -> dict of device tensors with
    ``ops.rasterize_mesh``'s keys: ``tri_id`` [B,H,W] int32 (-1 = empty),
    ``depth`` [B,H,W] float32 z-depth (the ray parameter of the unit direction
    over the direction's norm before normalisation; 0 = empty), ``label``
    [B,H,W] int32 (the label of the hit face's corner with the largest weight,
    the first on a tie; 0 = empty or no labels) and, if the mesh has ``rgb``,
    ``rgb`` [B,H,W,3] (barycentric blend).  A hit counts with z-depth in
    [``near``, ``far``].  ``batch`` views are cast per launch."""
    verts, faces = _dev_mesh(mesh, device)
    dev = verts.device
    if grid is None:
        grid = ops.triangle_grid(verts, faces)
    labels = None if mesh.get("labels") is None else \
        torch.as_tensor(np.asarray(mesh["labels"])).to(dev).to(torch.int32)
    rgb = None if mesh.get("rgb") is None else \
        torch.as_tensor(np.asarray(mesh["rgb"], np.float32)).to(dev)
    poses = torch.as_tensor(np.asarray(poses, np.float32) if not torch.is_tensor(poses) else poses)
    B, H, W = int(poses.shape[0]), int(H), int(W)
    out = {"tri_id": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "depth": torch.empty(B, H, W, device=dev),
           "label": torch.zeros(B, H, W, dtype=torch.int32, device=dev)}
    if rgb is not None:
        out["rgb"] = torch.zeros(B, H, W, 3, device=dev)
    for a in range(0, B, int(batch)):
        p = poses[a:a + batch].to(dev).float()
        b = int(p.shape[0])
        o, d, nrm = ops.get_rays(p, intrinsics, H, W)
        nrm = nrm.reshape(-1)
        face, t, bary = ops.raycast.raycast_mesh(grid, o.reshape(-1, 3), d.reshape(-1, 3),
                                                 nrm * float(near), nrm * float(far),
                                                 sort_rays=sort_rays)
        hit = face >= 0
        out["tri_id"][a:a + b] = face.view(b, H, W)
        out["depth"][a:a + b] = torch.where(hit, t / nrm, torch.zeros_like(t)).view(b, H, W)
        if faces.shape[0] and (labels is not None or rgb is not None):
            tri = faces[face.clamp_min(0).long()].long()                 # [n,3]
            if labels is not None:
                vert = tri.gather(1, bary.argmax(1, keepdim=True))[:, 0]
                out["label"][a:a + b] = torch.where(hit, labels[vert],
                                                    torch.zeros_like(face)).view(b, H, W)
            if rgb is not None:
                c = (rgb[tri] * bary[:, :, None]).sum(1)
                out["rgb"][a:a + b] = torch.where(hit[:, None], c,
                                                  torch.zeros_like(c)).view(b, H, W, 3)
    return out


def visible_points(grid, points, poses, intrinsics, H, W, near, far, bias, batch=16):
    """For each of ``points`` [N,3] (float32 on the GPU) the number of views that
    see it -> int32 [N] on the device.  A view with camera-to-world ``pose`` and
    centre C sees P if P's z-depth lies in [``near``, ``far``] (and is > 0), P
    projects inside the ``H`` x ``W`` image by ``ops.get_rays``' pixel convention
    (0 <= fx x/z + cx < W, 0 <= fy y/z + cy < H) and the segment from C towards P
    is free up to ``bias`` (scene units) before P:
    ``mesh_occluded(grid, C, P - C, 0, 1 - bias / |P - C|)`` is 0.  ``grid`` is
    ``ops.triangle_grid``'s dict of the occluding mesh.  The projection is
    elementwise torch, ``batch`` views at a time; only the points inside a
    view's frustum are cast."""
    pts = points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points, np.float32))
    pts = pts.to(device="cuda", dtype=torch.float32).reshape(-1, 3).contiguous() \
        if not pts.is_cuda else pts.float().reshape(-1, 3).contiguous()
    dev = pts.device
    poses = torch.as_tensor(np.asarray(poses, np.float32) if not torch.is_tensor(poses) else poses)
    poses = poses.to(dev).float().reshape(-1, 4, 4)
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    near, far, bias = float(near), float(far), float(bias)
    if not bias >= 0 or math.isnan(near) or math.isnan(far):
        raise ValueError(f"visible_points: bias must be >= 0 and near, far numbers, got "
                         f"{bias}, {near}, {far}")
    n = int(pts.shape[0])
    count = torch.zeros(n, dtype=torch.int32, device=dev)
    for a in range(0, int(poses.shape[0]), int(batch)):
        p = poses[a:a + batch]
        R, C = p[:, :3, :3], p[:, :3, 3]                                 # [b,3,3], [b,3]
        rel = pts[None, :, :] - C[:, None, :]                            # [b,N,3]
        cam = torch.einsum("bnr,brc->bnc", rel, R)                       # R^T (P - C)
        z = cam[..., 2]
        ok = (z > 0) & (z >= near) & (z <= far)
        zs = torch.where(ok, z, torch.ones_like(z))
        u, v = fx * cam[..., 0] / zs + cx, fy * cam[..., 1] / zs + cy
        ok &= (u >= 0) & (u < float(W)) & (v >= 0) & (v < float(H))
        view, idx = torch.nonzero(ok, as_tuple=True)
        if idx.numel() == 0:
            continue
        d = rel[view, idx].contiguous()
        t_max = 1.0 - bias / d.norm(dim=1)
        occ = ops.raycast.mesh_occluded(grid, C[view].contiguous(), d, 0.0, t_max.contiguous())
        count.index_add_(0, idx[occ == 0], torch.ones(int((occ == 0).sum()), dtype=torch.int32,
                                                      device=dev))
    return count
