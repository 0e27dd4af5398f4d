"""Helpers around ``SemanticNeRFNetwork.extract_semantic_mesh``: the 3D
semantic score against a labelled ground-truth mesh, and the frame maps.

Frames.  The field lives in the NGP frame: ``nerf_matrix_to_ngp`` takes a pose
of ``transforms_train.json`` (written by the reference's
``preprocessing_scripts/scannet2nerf.py``) and permutes its rows (y, z, x), so
a point p of the JSON frame sits at (p_y, p_z, p_x) in the field.  The JSON
translations are in scene units: metres times ``one_m_to_scene_uom``.
``ngp_to_pose_frame`` undoes both exactly (a permutation and one division).

How far back toward ScanNet's own frame that goes: scannet2nerf.py builds the
JSON poses from ScanNet's camera-to-world poses by (1) subtracting a room
centre (the bounding-box centre of ``*_vh_clean.ply`` with ``--room_center``,
else zero), (2) the fixed axis change (x, y, z) -> (y, x, -z), (3) a rotation
taking the mean camera up vector to +z, (4) without ``--room_center``,
subtracting the point the cameras look at, and (5) scaling by
``one_m_to_scene_uom``.  Only (5) is stored in the JSON; the rotation of (3)
and the offsets of (1) and (4) are printed, not saved.  So the mesh mapped by
``ngp_to_pose_frame`` is in metres and differs from ScanNet's frame by a rigid
motion (rotation + translation, no scale, no reflection) that the JSON does not
record: recompute it from ScanNet's pose files as scannet2nerf.py does, or
register the two meshes, before comparing them vertex by vertex."""
from __future__ import annotations

import numpy as np
import torch

from .metrics import SemanticsMeter


def ngp_to_pose_frame(verts, one_m_to_scene_uom=None):
    """NGP-frame points [V,3] -> the frame of transforms_train.json's poses
    (inverse of nerf_matrix_to_ngp's row permutation); in metres when
    ``one_m_to_scene_uom`` is given, else in scene units."""
    v = np.asarray(verts)
    out = v[:, [2, 0, 1]].astype(np.float64)
    if one_m_to_scene_uom is not None:
        out = out / float(one_m_to_scene_uom)
    return out


def pose_frame_to_ngp(points, one_m_to_scene_uom=None):
    """The inverse of ``ngp_to_pose_frame``: points of the transforms JSON frame
    (metres when ``one_m_to_scene_uom`` is given) -> NGP frame, float32."""
    p = np.asarray(points, np.float64)
    if one_m_to_scene_uom is not None:
        p = p * float(one_m_to_scene_uom)
    return p[:, [1, 2, 0]].astype(np.float32)


@torch.no_grad()
def evaluate_semantic_mesh(net, verts, gt_labels, chunk=1 << 20):
    """3D semantic score of a field against a labelled mesh.  ``verts`` [V,3]
    are the ground-truth vertices in the field's (NGP) frame, ``gt_labels`` [V]
    NYU40 ids as in ScanNet's labels.ply (0 = unknown, ignored; 1..C map to the
    classes 0..C-1).  The field's class at each vertex is the argmax of
    ``net.semantics`` on ``net.density(verts)["geo_feat"]``; the confusion matrix
    is ``ops.confusion_matrix`` through ``SemanticsMeter``.
    -> {"mIoU", "total_acc", "mean_acc"} (SemanticsMeter.measure)."""
    dev = net.encoder.params.device
    C = net.num_semantic_classes
    v = torch.as_tensor(np.asarray(verts, np.float32)).to(dev)
    gt = torch.as_tensor(np.asarray(gt_labels).astype(np.int64)).to(dev)
    truth = torch.where((gt >= 1) & (gt <= C), gt - 1, torch.full_like(gt, -1))
    meter = SemanticsMeter(C)
    for a in range(0, v.shape[0], chunk):
        b = min(v.shape[0], a + chunk)
        geo = net.density(v[a:b])["geo_feat"].contiguous()
        pred = net.semantics(None, None, geo_feat=geo).argmax(-1)
        meter.update(pred, truth[a:b])
    miou, total_acc, mean_acc = meter.measure()
    return {"mIoU": miou, "total_acc": total_acc, "mean_acc": mean_acc}
