"""Per-frame 2D label maps fused onto a mesh by multi-view voting, on the GPU:
the mapping-based pseudo-label baseline (frame predictions -> 3D map -> frames)
out of the project's own parts.

    label maps --fuse_views--> vertex labels --ops.rasterize_mesh--> map_label

Every pixel of every view votes for the mesh vertex that the rasterizer gives it
(``ops.rasterize_mesh`` with ``vertex_labels = 1..V``: the nearest corner of the
hit point) with its frame's class; ``ops.fuse_label_votes`` sums the votes in a
uint64 table that stays on the device, ``ops.resolve_label_votes`` takes the
majority.  With ``score_maps`` (rows of evidence codes per pixel,
``ops.log_evidence``) a pixel adds its row to its vertex instead
(``ops.fuse_label_evidence``, same table) and the majority becomes the MAP
class.  With ``smooth`` the table is pooled over each vertex's edge neighbours
before it is resolved (``ops.smooth_label_table``), which also fills unobserved
vertices from their neighbours.  ``simplify_mesh`` makes a mesh coarser by
vertex clustering before (or after) fusing, and ``pool_label_table`` carries a
table fused on the fine mesh to the coarse one.  Out of scope: float probabilities on the
device, priors, registering a
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


def _score_batch(src, a, b, H, W, C):
    """views a..b of ``src`` as one uint8 [b-a,H,W,C] tensor; a view is [H,W,C] or
    [C,H,W], told apart by shape ([H,W,C] where both fit)"""
    out = []
    for i in range(a, b):
        arr = np.asarray(_view(src, i))
        if arr.dtype != np.uint8:
            raise ValueError(f"score_maps: views must be uint8, got {arr.dtype}")
        if arr.shape == (C, H, W) and arr.shape != (H, W, C):
            arr = arr.transpose(1, 2, 0)
        if arr.shape != (H, W, C):
            raise ValueError(f"score_maps: views must be [{H},{W},{C}] or [{C},{H},{W}], got "
                             f"{arr.shape}")
        out.append(arr)
    return torch.from_numpy(np.ascontiguousarray(np.stack(out)))


def fuse_views(mesh, poses, intrinsics, H, W, near, label_maps, depth_maps=None,
               depth_tol=None, weights=None, num_classes=40, batch=16, min_votes=1,
               device="cuda", score_maps=None, min_margin=0, smooth=0):
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
    ``rasterize_ms`` / ``accumulate_ms`` (device-synchronised host clock).
    With ``score_maps`` (``i -> [H,W,C]`` or ``[C,H,W]`` uint8 evidence codes,
    C = ``num_classes``; ``label_maps`` is then not read and may be None,
    ``weights`` must be None) a pixel adds its row of codes instead of one
    vote; ``total`` / ``winner`` and ``min_votes`` are then in evidence units,
    the dict carries ``margin`` [V] uint64 (the winner's lead over the
    runner-up; the winner itself for one class) and a vertex whose margin is
    below ``min_margin`` gets label 0.
    ``smooth`` = N > 0 pools the table N times over each vertex's edge
    neighbours (``ops.mesh_adjacency`` / ``ops.smooth_label_table``) before it
    is resolved: an unobserved vertex takes its neighbours' label, and
    ``min_votes`` / ``min_margin`` count pooled units.  0 leaves everything as
    it was."""
    smooth = int(smooth)
    if smooth < 0:
        raise ValueError("smooth must be >= 0")
    soft = score_maps is not None
    if not soft and min_margin:
        raise ValueError("min_margin applies to score_maps only")
    if soft and weights is not None:
        raise ValueError("weights apply to label_maps only")
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
        if soft:
            sc = _score_batch(score_maps, a, b, H, W, int(num_classes)).to(dev)
        else:
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
        if soft:
            ops.fuse_label_evidence(votes, out["label"], sc,
                                    mesh_depth=None if sd is None else out["depth"],
                                    sensor_depth=sd, depth_tol=depth_tol)
        else:
            ops.fuse_label_votes(votes, out["label"], pred, weight=w,
                                 mesh_depth=None if sd is None else out["depth"],
                                 sensor_depth=sd, depth_tol=depth_tol)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        t_r += t1 - t0
        t_a += t3 - t2
    if smooth:
        votes = ops.smooth_label_table(votes, ops.mesh_adjacency(faces, V), iterations=smooth)
    res = ops.resolve_label_votes(votes, min_votes)
    extra = {}
    if soft:
        top = votes[:, 1:].topk(min(2, votes.shape[1] - 1), dim=1).values
        margin = top[:, 0] - top[:, 1] if top.shape[1] == 2 else top[:, 0]
        res["label"] = torch.where(margin >= int(min_margin), res["label"],
                                   torch.zeros_like(res["label"]))
        extra["margin"] = margin.cpu().numpy().view(np.uint64)
    labels = res["label"].cpu().numpy()
    return {**extra, "labels": labels,
            "total": res["total"].cpu().numpy().view(np.uint64),
            "winner": res["winner"].cpu().numpy().view(np.uint64),
            "observed": int((labels > 0).sum()),
            "rasterize_ms": 1e3 * t_r, "accumulate_ms": 1e3 * t_a}


def filter_mesh_components(mesh, min_vertices=0, keep_largest=None, device="cuda"):
    """Drop the small connected components of a mesh: the floaters of a
    reconstruction.  ``mesh`` is a dict as ``load_mesh`` gives it (numpy: verts
    [V,3], faces [F,3] int32, optional normals / rgb / labels per vertex).  Kept
    are the components (over the mesh's edges; a vertex no face uses is a
    component of one) with at least ``min_vertices`` vertices and, if
    ``keep_largest`` = K is given, among the K with the most vertices, ties
    going to the component with the smaller label (its smallest vertex index).
    -> (new dict, statistics): verts, normals, rgb and labels compacted, faces
    renumbered, surviving vertices and faces in their former relative order,
    every other entry passed on, plus ``vertex_index`` / ``face_index`` (int64:
    which of the input's vertices and faces survive);
    {"components": n, "removed_components": m, "removed_vertices": k,
    "largest": s}.  The labelling runs in the kernels (``ops.mesh_adjacency``,
    ``ops.mesh_components``, ``ops.component_sizes``); the compaction is torch
    indexing."""
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError("keep_largest must be >= 1")
    dev = torch.device(device)
    verts = np.asarray(mesh["verts"])
    V = int(verts.shape[0])
    faces = torch.from_numpy(np.ascontiguousarray(mesh["faces"], np.int32)).to(dev)
    labels = ops.mesh_components(ops.mesh_adjacency(faces, V))
    sizes = ops.component_sizes(labels).long()
    ids = torch.arange(V, device=dev)
    roots = ids[labels.long() == ids]                      # ascending: by label
    root_sizes = sizes[roots]
    keep_root = root_sizes >= int(min_vertices)
    if keep_largest is not None:
        # by size, largest first; a stable sort keeps equal sizes in label order
        order = torch.sort(root_sizes, descending=True, stable=True).indices
        top = torch.zeros_like(keep_root)
        top[order[:int(keep_largest)]] = True
        keep_root &= top
    keep_label = torch.zeros(V, dtype=torch.bool, device=dev)
    keep_label[roots[keep_root]] = True
    keep_v = keep_label[labels.long()] if V else keep_label
    new_id = torch.cumsum(keep_v.long(), 0) - 1
    fl = faces.long()
    keep_f = keep_v[fl].all(1) if fl.numel() else torch.zeros(0, dtype=torch.bool, device=dev)
    new_faces = new_id[fl[keep_f]].to(torch.int32)
    vi, fi = ids[keep_v].cpu().numpy(), torch.nonzero(keep_f).view(-1).cpu().numpy()
    out = dict(mesh)
    for k in ("verts", "normals", "rgb", "labels"):
        if mesh.get(k) is not None:
            out[k] = np.ascontiguousarray(np.asarray(mesh[k])[vi])
    out["faces"] = new_faces.cpu().numpy().reshape(-1, 3)
    out["vertex_index"], out["face_index"] = vi, fi
    gone = ~keep_root
    stats = {"components": int(roots.numel()), "removed_components": int(gone.sum()),
             "removed_vertices": int(root_sizes[gone].sum()),
             "largest": int(root_sizes.max()) if roots.numel() else 0}
    return out, stats


def simplify_mesh(mesh, cell, split_labels=False, device="cuda"):
    """Simplify a mesh by vertex clustering (``ops.simplify_mesh``): the vertices
    of one cell of a grid of edge ``cell`` become one vertex, so the mesh comes
    out about as fine as ``cell``.  ``mesh`` is a dict as ``load_mesh`` gives it
    (numpy: verts [V,3], faces [F,3] int32, optional normals / rgb / labels per
    vertex; rgb uint8, or float in [0,1], which is rounded to 0..255 for the
    averaging and returned as float again; labels 0..255).  With
    ``split_labels`` vertices of different labels are never merged.  -> (new
    dict, statistics): verts, faces, normals, rgb and labels replaced (dtypes
    kept), ``face_classes`` [F], if present, indexed by ``face_index``, every
    other entry passed on, plus ``vertex_map`` (int32 [V]: the output vertex of
    every input vertex, -1 for a non-finite one) and ``face_index`` (int32: the
    input face of every output face); {"vertices": [in, out], "faces": [in,
    out], "degenerate": k, "duplicate": d, "largest_cluster": m}."""
    dev = torch.device(device)
    put = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    verts = put(np.asarray(mesh["verts"]).reshape(-1, 3), np.float32)
    faces = put(np.asarray(mesh["faces"]).reshape(-1, 3), np.int32)
    normals = rgb = labels = None
    if mesh.get("normals") is not None:
        normals = put(np.asarray(mesh["normals"]).reshape(-1, 3), np.float32)
    if mesh.get("rgb") is not None:
        c = np.asarray(mesh["rgb"]).reshape(-1, 3)
        if c.dtype != np.uint8:      # write_ply's rounding
            c = np.round(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)
        rgb = put(c, np.uint8)
    if mesh.get("labels") is not None:
        labels = put(np.asarray(mesh["labels"]).reshape(-1), np.int64)
    res = ops.simplify_mesh(verts, faces, cell, normals=normals, rgb=rgb, labels=labels,
                            split_labels=split_labels)
    out = dict(mesh)
    out["verts"] = res["verts"].cpu().numpy()
    out["faces"] = res["faces"].cpu().numpy().reshape(-1, 3)
    if normals is not None:
        out["normals"] = res["normals"].cpu().numpy().astype(np.asarray(mesh["normals"]).dtype)
    if rgb is not None:
        c = res["rgb"].cpu().numpy()
        src = np.asarray(mesh["rgb"])
        out["rgb"] = c if src.dtype == np.uint8 else \
            (c.astype(np.float32) / np.float32(255.0)).astype(src.dtype)
    if labels is not None:
        out["labels"] = res["labels"].cpu().numpy().astype(np.asarray(mesh["labels"]).dtype)
    out["vertex_map"] = res["vertex_map"].cpu().numpy()
    out["face_index"] = res["face_index"].cpu().numpy()
    if mesh.get("face_classes") is not None:
        out["face_classes"] = np.asarray(mesh["face_classes"])[out["face_index"]]
    count = res["count"]
    stats = {"vertices": [int(verts.shape[0]), int(count.numel())],
             "faces": [int(faces.shape[0]), int(out["faces"].shape[0])],
             "degenerate": int(res["degenerate"]), "duplicate": int(res["duplicate"]),
             "largest_cluster": int(count.max()) if count.numel() else 0}
    return out, stats


def pool_label_table(votes, vertex_map, n_out):
    """Carry a vote or evidence table from a fine mesh to its simplified one:
    ``votes`` [V, C+1] int64 on the GPU (the bits of the uint64 table of
    ``ops.fuse_label_votes`` / ``ops.fuse_label_evidence``), ``vertex_map`` [V]
    (``simplify_mesh``'s: the coarse vertex of every fine one, -1 = none) -> a
    NEW [n_out, C+1] int64 table: row k is the sum of the rows mapped to k,
    exact modulo 2^64 (integer adds, so the order does not matter); -1 rows are
    skipped.  ``ops.resolve_label_votes`` reads the result as it is.  The table
    is not modified.  ``index_add_`` on the device: plumbing, not a kernel."""
    if not (torch.is_tensor(votes) and votes.dtype == torch.int64 and votes.dim() == 2):
        raise ValueError("votes must be an int64 [V, C+1] tensor")
    vm = torch.as_tensor(np.asarray(vertex_map) if not torch.is_tensor(vertex_map)
                         else vertex_map).to(votes.device).long().view(-1)
    if vm.numel() != votes.shape[0]:
        raise ValueError(f"vertex_map has {vm.numel()} entries, the table {votes.shape[0]} rows")
    n_out = int(n_out)
    if vm.numel() and (int(vm.min()) < -1 or int(vm.max()) >= n_out):
        raise ValueError(f"vertex_map must lie in -1..{n_out - 1}")
    out = torch.zeros((n_out, votes.shape[1]), dtype=torch.int64, device=votes.device)
    keep = vm >= 0
    out.index_add_(0, vm[keep], votes[keep])
    return out
