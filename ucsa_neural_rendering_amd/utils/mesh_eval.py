"""3D scores of fused maps (``ops.point_grid`` + ``ops.nearest_point``): labels
carried from one vertex set to another by nearest neighbour, the label score of
a fused mesh or voxel map at the vertices of a ground-truth mesh (ScanNet's
protocol: the vertices of ``*_vh_clean_2.labels.ply`` take the label of the
nearest predicted vertex), and the geometric score of a mesh against another
(accuracy, completeness, chamfer, precision / recall / F-score).

Meshes come as ``utils.mesh_render.load_mesh`` returns them, both in one frame
(numpy or tensors; labels are NYU40 ids: class + 1, 0 = unknown).  Finding the
rigid motion between two frames is not done here.  ``max_dist`` is required: a
vertex with nothing within it is unmatched, and a query with nothing near costs
the walk over every cell within ``max_dist``.

Vertex to vertex is right only when both meshes are tessellated about equally
finely.  Where the target's faces are given (``src_faces``, ``pred_faces``,
``gt_faces``) the search is for the nearest point on its surface instead
(``ops.triangle_grid`` + ``ops.nearest_triangle``): a vertex in the middle of a
large ground-truth triangle is then at distance 0, not half an edge away.

That settles the target.  The query points are a mesh's vertices unless
``sample_density`` is given: then they are drawn from the mesh's surface
(``ops.sample_mesh_surface``: so many points per unit area, deterministic for a
``seed``), so that a wall of two triangles weighs by its area and not by its
four corners, and a hole in the middle of it costs what it covers.

``voxel_iou`` is the score that depends neither on tessellation nor on a
distance threshold: both meshes are voxelized on one lattice
(``ops.voxelize_mesh``) and the occupied voxel sets are compared.

A scene fused from some of its frames has seen part of the room only.
``visible_from`` (``mesh_distance``, ``score_labels_3d``) restricts the
ground-truth side's points to those that at least ``min_views`` of the given
cameras see (``utils.mesh_raycast.visible_points``: inside the image and the
depth range, the segment from the camera free of the ground-truth mesh), so
that completeness, recall and the label score no longer charge for surface no
camera observed.

All of these are unsigned.  ``mesh_distance(signed=True)`` and ``tsdf_bias`` say
on which side of the ground-truth surface a mesh or a fused volume lies
(``ops.signed_distance``, ``ops.mesh_tsdf``): an inflated surface and a deflated
one score the same everywhere else."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops
from .mesh_render import score_label_maps


def _verts(v, device="cuda"):
    t = torch.as_tensor(np.asarray(v, np.float32) if not torch.is_tensor(v) else v)
    return t.to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()


def _labels(l, n, device):
    t = torch.as_tensor(np.asarray(l) if not torch.is_tensor(l) else l).reshape(-1)
    if t.numel() != n:
        raise ValueError(f"{t.numel()} labels for {n} vertices")
    return t.to(device=device, dtype=torch.int32)


def _faces(f, device):
    t = torch.as_tensor(np.asarray(f) if not torch.is_tensor(f) else f)
    return t.to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()


def _seen(points, gt, gt_faces, visible_from, min_views):
    """which of ``points`` at least ``min_views`` of the views of ``visible_from``
    (a dict of poses, intrinsics, H, W, near, far, bias) see, the ground-truth
    mesh being the occluder -> bool [N] on the device"""
    from .mesh_raycast import visible_points
    if gt_faces is None:
        raise ValueError("visible_from needs gt_faces: the ground-truth mesh is the occluder")
    try:
        keys = {k: visible_from[k] for k in ("poses", "intrinsics", "H", "W", "near", "far",
                                              "bias")}
    except (TypeError, KeyError):
        raise ValueError("visible_from must be a dict of poses, intrinsics, H, W, near, far, bias")
    grid = ops.triangle_grid(gt, _faces(gt_faces, gt.device))
    return visible_points(grid, points, **keys) >= int(min_views)


def sample_surface(verts, faces, density, seed=0, labels=None, samples=None):
    """Query points on a mesh's surface (``ops.sample_mesh_surface``) -> (points
    float32 [S,3] on the device, labels int32 [S] or None, the op's dict).
    ``labels`` [V] (0..255) are carried to the samples: each takes the label of
    its face's corner with the largest weight.  ``samples=N`` instead of a
    density asks for about N points: density = N / sum(area), the sum taken in
    float64 on the host from the op's ``area`` array."""
    v = _verts(verts)
    f = _faces(faces, v.device)
    lab = None if labels is None else _labels(labels, v.shape[0], v.device)
    if (density is None) == (samples is None):
        raise ValueError("give one of density and samples")
    if density is None:
        area = ops.sample_mesh_surface(v, f, 1.0, seed, max_samples=1 << 31)["area"]
        total = float(np.sum(area.cpu().numpy(), dtype=np.float64))
        if not total > 0:
            raise ValueError("the mesh has no area to put samples on")
        density = float(samples) / total
    res = ops.sample_mesh_surface(v, f, density, seed, labels=lab)
    got = None if lab is None else res["labels"].to(torch.int32)
    return res["points"], got, res


def transfer_labels(src_verts, src_labels, dst_verts, max_dist, return_match=False,
                    src_faces=None):
    """The label of the nearest ``src`` vertex within ``max_dist`` at every ``dst``
    vertex -> int32 [D] on the device; 0 where there is none.  Among equally near
    source vertices the smallest index decides.  ``return_match``: also the
    ``index`` (-1 = none) and ``dist2`` of ``ops.nearest_point``.

    With ``src_faces`` [F,3] the nearest point of the source's surface decides:
    every ``dst`` vertex takes the label of the corner with the largest
    barycentric weight of its nearest face (the first such corner on a tie), and
    ``return_match`` gives (labels, ``index`` of that corner's vertex, ``dist2``,
    ``face``, ``bary``) of ``ops.nearest_triangle``."""
    src = _verts(src_verts)
    dst = _verts(dst_verts, src.device)
    lab = _labels(src_labels, src.shape[0], src.device)
    if src_faces is not None:
        faces = _faces(src_faces, src.device)
        face, dist2, bary = ops.nearest_triangle(ops.triangle_grid(src, faces), dst, max_dist)
        hit = face >= 0
        out = torch.zeros(dst.shape[0], dtype=torch.int32, device=src.device)
        index = torch.full_like(face, -1)
        if faces.shape[0] and lab.numel():
            corner = bary.argmax(1, keepdim=True)                   # the first maximum
            vert = faces[face.clamp_min(0).long()].gather(1, corner)[:, 0]
            index = torch.where(hit, vert, index)
            out = torch.where(hit, lab[vert.clamp(0, src.shape[0] - 1).long()], out)
        return (out, index, dist2, face, bary) if return_match else out
    index, dist2 = ops.nearest_point(ops.point_grid(src), dst, max_dist)
    hit = index >= 0
    out = torch.zeros(dst.shape[0], dtype=torch.int32, device=src.device)
    if lab.numel():
        out = torch.where(hit, lab[index.clamp_min(0).long()], out)
    return (out, index, dist2) if return_match else out


def _score(pred, index, gt_labels, C):
    gt = torch.as_tensor(np.asarray(gt_labels) if not torch.is_tensor(gt_labels)
                         else gt_labels).reshape(-1).to(pred.device)
    if gt.numel() != pred.numel():
        raise ValueError(f"{gt.numel()} ground-truth labels for {pred.numel()} vertices")
    s = score_label_maps(pred.cpu().numpy(), gt.cpu().numpy(), C)
    scored = (gt >= 1) & (gt <= C)
    n = int(scored.sum())
    return {"mIoU": s["mIoU"], "total_acc": s["total_acc"], "mean_acc": s["mean_acc"],
            "vertices": n,
            "unmatched": float(((index < 0) & scored).sum()) / n if n else float("nan")}


def score_labels_3d(pred_verts, pred_labels, gt_verts, gt_labels, max_dist, C=40,
                    pred_faces=None, gt_faces=None, sample_density=None, seed=0,
                    visible_from=None, min_views=1):
    """The predicted labels at the ground-truth vertices (``transfer_labels``)
    scored through ``score_label_maps``: ground truth 0 or above ``C`` is ignored;
    a prediction of 0, or no predicted vertex within ``max_dist``, counts as
    wrong, exactly as the 2D score treats it.  -> {"mIoU", "total_acc",
    "mean_acc", "vertices" (scored), "unmatched" (the share of scored vertices
    without a match)}.  ``pred_faces``: the labels come from the nearest point of
    the predicted surface (``transfer_labels`` with ``src_faces``).

    ``gt_faces`` with ``sample_density``: the score is taken at points sampled
    from the ground-truth surface (``sample_surface``, ``seed``), each carrying
    the label of its face's nearest corner, and so weighs every class by its
    area; "vertices" is then the number of scored samples and "sampled" the
    number of samples.

    ``visible_from`` (a dict of poses, intrinsics, H, W, near, far, bias; needs
    ``gt_faces``, the occluder): only the ground-truth vertices or samples that at
    least ``min_views`` of those views see (``visible_points``) are scored, and
    the dict gains "visible": [kept, total]."""
    if visible_from is not None and gt_faces is None:
        raise ValueError("visible_from needs gt_faces: the ground-truth mesh is the occluder")
    if sample_density is None:
        points, labels = gt_verts, gt_labels
    else:
        if gt_faces is None:
            raise ValueError("sample_density needs gt_faces")
        points, labels, res = sample_surface(gt_verts, gt_faces, sample_density, seed, gt_labels)
    visible = None
    if visible_from is not None:
        gt = _verts(gt_verts)
        points = _verts(points, gt.device)
        labels = _labels(labels, points.shape[0], gt.device)
        keep = _seen(points, gt, gt_faces, visible_from, min_views)
        visible = [int(keep.sum()), int(keep.numel())]
        points, labels = points[keep].contiguous(), labels[keep]
    pred, index = transfer_labels(pred_verts, pred_labels, points, max_dist,
                                  return_match=True, src_faces=pred_faces)[:2]
    out = _score(pred, index, labels, C)
    if sample_density is not None:
        out["sampled"] = res["n_samples"]
    if visible is not None:
        out["visible"] = visible
    return out


def voxel_centres(volume, voxel_labels):
    """-> (centres float32 [M,3], labels int32 [M]) of the voxels whose label is
    > 0, on the device: ``origin + index * spacing`` in float32."""
    lab = torch.as_tensor(voxel_labels)
    if tuple(lab.shape) != tuple(volume["tsdf"].shape):
        raise ValueError(f"voxel_labels {tuple(lab.shape)} against a volume of "
                         f"{tuple(volume['tsdf'].shape)}")
    lab = lab.to(volume["tsdf"].device)
    ijk = torch.nonzero(lab > 0)
    origin = torch.tensor(volume["origin"], dtype=torch.float32, device=lab.device)
    spacing = torch.tensor(volume["spacing"], dtype=torch.float32, device=lab.device)
    centres = origin[None, :] + ijk.to(torch.float32) * spacing[None, :]
    return centres, lab[ijk[:, 0], ijk[:, 1], ijk[:, 2]].to(torch.int32)


def score_voxel_labels_3d(volume, voxel_labels, gt_verts, gt_labels, max_dist, C=40,
                          gt_faces=None, sample_density=None, seed=0):
    """``score_labels_3d`` with the centres of the labelled voxels of a voxel map
    (``utils.voxel_map``: the volume and its resolved labels) as the predicted
    point set; ``gt_faces``, ``sample_density`` and ``seed`` as there."""
    centres, lab = voxel_centres(volume, voxel_labels)
    return score_labels_3d(centres, lab, gt_verts, gt_labels, max_dist, C, gt_faces=gt_faces,
                           sample_density=sample_density, seed=seed)


def mesh_distance(pred_verts, gt_verts, threshold, max_dist, pred_faces=None, gt_faces=None,
                  sample_density=None, seed=0, signed=False, visible_from=None, min_views=1):
    """Vertex-to-vertex distances both ways -> {"accuracy": mean pred -> gt,
    "completeness": mean gt -> pred, "chamfer": their mean, "precision": the share
    of pred vertices within ``threshold`` of gt, "recall": the share of gt
    vertices within ``threshold`` of pred, "fscore": their harmonic mean (0 when
    both are 0)}.  Distances are ``sqrt(dist2)`` in float64 on the device; a
    vertex with nothing within ``max_dist`` counts as ``max_dist`` (and is not
    within the threshold).  An empty set gives nan for its direction.

    A direction whose target has faces measures vertex to surface: ``gt_faces``
    [F,3] the pred -> gt direction (accuracy, precision), ``pred_faces`` the
    gt -> pred direction (completeness, recall).  With either given the dict
    also holds "surface": (pred -> gt is to the surface, gt -> pred is).

    ``sample_density``: a side that has faces is measured from points sampled on
    its surface at that density (``sample_surface``, ``seed``) instead of from
    its vertices: pred -> gt from the samples of ``pred_faces``, gt -> pred from
    those of ``gt_faces``.  Recall then falls by the share of the ground-truth
    area that the predicted mesh leaves uncovered.  The dict also holds
    "sampled": [n_pred, n_gt], the number of samples on each side (0 for a side
    without faces, which is measured from its vertices).

    ``signed`` (needs ``gt_faces``): the pred -> gt direction is
    ``ops.signed_distance`` and the dict gains, over the matched points only, in
    float64 on the device, "signed_mean" and "signed_median" (the median is the
    lower one) of the signed distance and "behind_share", the share with a
    negative one; nan when nothing matched.  Positive is the side the
    ground-truth faces' (B-A)x(C-A) points to: for a ground truth that is
    counter-clockwise seen from outside, a positive mean is an inflated
    prediction and a negative one a deflated one.  Every other entry is what it
    is without the keyword.

    ``visible_from`` (a dict of poses, intrinsics, H, W, near, far, bias; needs
    ``gt_faces``, the occluder): the gt -> pred direction (completeness, recall)
    is measured only from the ground-truth vertices or samples that at least
    ``min_views`` of those views see (``visible_points``); the dict gains
    "visible": [kept, total].  The pred -> gt direction still has the whole
    ground truth as its target."""
    pred = _verts(pred_verts)
    gt = _verts(gt_verts, pred.device)
    if visible_from is not None and gt_faces is None:
        raise ValueError("visible_from needs gt_faces: the ground-truth mesh is the occluder")
    if signed and gt_faces is None:
        raise ValueError("mesh_distance: signed needs gt_faces")
    signed_out = {}
    pred_from, gt_from, sampled = pred, gt, [0, 0]
    if sample_density is not None:
        if pred_faces is not None:
            pred_from, _, res = sample_surface(pred, pred_faces, sample_density, seed)
            sampled[0] = res["n_samples"]
        if gt_faces is not None:
            gt_from, _, res = sample_surface(gt, gt_faces, sample_density, seed)
            sampled[1] = res["n_samples"]
    visible = None
    if visible_from is not None:
        keep = _seen(gt_from, gt, gt_faces, visible_from, min_views)
        visible = [int(keep.sum()), int(keep.numel())]
        gt_from = gt_from[keep].contiguous()

    def one_way(a, b, b_faces, with_sign=False):
        if with_sign:
            signed_out.update(signed_mean=float("nan"), signed_median=float("nan"),
                              behind_share=float("nan"))
        if a.shape[0] == 0:
            return float("nan"), float("nan")
        if with_sign:
            fc = _faces(b_faces, b.device)
            sdf, index, dist2, _, _ = ops.signed_distance(
                ops.triangle_grid(b, fc), ops.mesh_pseudonormals(b, fc), b, fc, a, max_dist)
            s = sdf[index >= 0].double()
            if s.numel():
                signed_out.update(signed_mean=float(s.mean()),
                                  signed_median=float(s.median()),
                                  behind_share=float((s < 0).double().mean()))
        elif b_faces is not None:
            grid = ops.triangle_grid(b, _faces(b_faces, b.device))
            index, dist2, _ = ops.nearest_triangle(grid, a, max_dist)
        else:
            index, dist2 = ops.nearest_point(ops.point_grid(b), a, max_dist)
        d = torch.where(index >= 0, dist2.double().sqrt(),
                        torch.full_like(dist2, float(max_dist), dtype=torch.float64))
        return float(d.mean()), float(((index >= 0) & (d <= float(threshold))).double().mean())

    acc, prec = one_way(pred_from, gt, gt_faces, bool(signed))
    comp, rec = one_way(gt_from, pred, pred_faces)
    if not prec + rec >= 0:                         # an empty set: nan
        f = float("nan")
    elif prec + rec == 0:
        f = 0.0
    else:
        f = 2.0 * prec * rec / (prec + rec)
    out = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp),
           "precision": prec, "recall": rec, "fscore": f}
    if pred_faces is not None or gt_faces is not None:
        out["surface"] = (gt_faces is not None, pred_faces is not None)
    if sample_density is not None:
        out["sampled"] = sampled
    out.update(signed_out)
    if visible is not None:
        out["visible"] = visible
    return out


def voxel_iou(pred_verts, pred_faces, gt_verts, gt_faces, voxel, dilate=0.0, aabb=None,
              max_voxels=1 << 28):
    """Volumetric IoU of the voxel sets two meshes pass through
    (``ops.voxelize_mesh``, surface voxelization: a cell counts when a face
    meets its box grown by ``dilate``).  The lattice is cubic with spacing
    ``voxel`` over the union box of the finite vertices of both meshes (or
    ``aabb`` [2,3]) padded by one voxel: origin = lo - voxel, dims =
    ceil((hi + voxel - origin) / voxel) + 1 per axis, in float32.  -> {"iou":
    |P & G| / |P | G| (1.0 when both are empty), "precision": |P & G| / |P|,
    "recall": |P & G| / |G| (1.0 for an empty denominator), "n_pred", "n_gt",
    "dims", "voxel"}.  More than ``max_voxels`` voxels is an error raised
    before anything of that size is allocated."""
    pred = _verts(pred_verts)
    gt = _verts(gt_verts, pred.device)
    voxel = float(np.float32(voxel))
    if not (voxel > 0 and np.isfinite(voxel)):
        raise ValueError(f"voxel must be > 0 and finite, got {voxel}")
    if aabb is None:
        pts = torch.cat([pred, gt])
        pts = pts[torch.isfinite(pts).all(1)]
        if pts.shape[0] == 0:
            raise ValueError("voxel_iou: no finite vertex and no aabb")
        box = torch.stack([pts.amin(0), pts.amax(0)]).cpu().numpy()
    else:
        box = np.asarray(aabb, np.float32).reshape(2, 3)
    v32 = np.float32(voxel)
    lo = (box[0] - v32).astype(np.float32)
    hi = (box[1] + v32).astype(np.float32)
    dims = tuple(int(np.ceil(float(hi[a] - lo[a]) / voxel)) + 1 for a in range(3))
    if dims[0] * dims[1] * dims[2] > min(int(max_voxels), 0x7FFFFFFF):
        raise ValueError(f"voxel {voxel} gives {dims} voxels, more than max_voxels = "
                         f"{max_voxels}: raise voxel")
    origin = [float(v) for v in lo]
    P = ops.voxelize_mesh(pred, _faces(pred_faces, pred.device), dims, origin, voxel, dilate) != 0
    G = ops.voxelize_mesh(gt, _faces(gt_faces, pred.device), dims, origin, voxel, dilate) != 0
    inter, n_p, n_g = int((P & G).sum()), int(P.sum()), int(G.sum())
    union = n_p + n_g - inter
    return {"iou": inter / union if union else 1.0, "precision": inter / n_p if n_p else 1.0,
            "recall": inter / n_g if n_g else 1.0, "n_pred": n_p, "n_gt": n_g,
            "dims": list(dims), "voxel": voxel}


def tsdf_bias(volume, gt_verts, gt_faces, trunc, min_weight=1.0):
    """The signed offset of a fused TSDF volume from a ground-truth mesh, voxel
    by voxel: ``ops.mesh_tsdf`` fills a scratch volume of the same lattice from
    the mesh, and over the voxels observed in both (``weight >= min_weight`` in
    ``volume``, inside the mesh's band of ``trunc``) the differences
    ``(tsdf - tsdf_gt) * trunc`` (scene units) give {"mean", "median" (the lower
    one), "mean_abs", "n"}; nan with n = 0 when no voxel is shared.  ``trunc``
    is the truncation ``volume`` was fused with.  A positive mean says the
    fused surface lies on the negative side of the mesh (behind it, for a mesh
    that is counter-clockwise seen from outside): the fused volume is
    deflated."""
    (nx, ny, nz), dev = ops.volume_lattice(volume)
    ref = ops.tsdf_volume((nx, ny, nz), volume["origin"], volume["spacing"], device=dev)
    ops.mesh_tsdf(ref, _verts(gt_verts, dev), _faces(gt_faces, dev), trunc, weight=1.0)
    both = (volume["weight"] >= float(min_weight)) & (ref["weight"] > 0)
    d = (volume["tsdf"][both].double() - ref["tsdf"][both].double()) * float(trunc)
    n = int(d.numel())
    if n == 0:
        return {"mean": float("nan"), "median": float("nan"), "mean_abs": float("nan"), "n": 0}
    return {"mean": float(d.mean()), "median": float(d.median()),
            "mean_abs": float(d.abs().mean()), "n": n}
