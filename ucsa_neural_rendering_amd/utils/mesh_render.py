"""Labelled meshes rendered into the project's posed frames (``ops.rasterize_mesh``):
mesh-rendered label / depth / colour images at the training poses or at the
predict pass's novel viewpoints, and their 2D score against pseudo-labels.

Frames.  Poses come from ``transforms_train.json`` (``frames[*].transform_matrix``)
or from ``<exp>/novel_viewpoints/interpolated_data.json`` (``frames[*].pose``,
written by the predict pass), both through ``nerf_matrix_to_ngp`` as the
dataset reads them; intrinsics and ``one_m_to_scene_uom`` from the transforms
JSON.  The mesh must be in the same (NGP) frame: ``load_mesh`` takes it there
from the frame of the JSON poses in metres (``pose_frame=True``, what
``scripts/export_semantic_mesh.py --one_m_to_scene_uom`` writes) with
``pose_frame_to_ngp``.  Rendered depth is z in scene units; divided by
``one_m_to_scene_uom`` it is metres, the unit of ``depth/*.png`` (millimetres)."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .. import ops
from ..dataset.ngp_utils import nerf_matrix_to_ngp
from .metrics import SemanticsMeter
from .ply import read_ply
from .semantic_mesh import pose_frame_to_ngp


def load_mesh(src, pose_frame=False, one_m_to_scene_uom=None):
    """A PLY path (``read_ply``: ScanNet's labels.ply or an exported mesh) or an
    ``extract_semantic_mesh`` dict -> dict of numpy arrays in the NGP frame:
    verts [V,3] f32, faces [F,3] int32, labels [V] int32 NYU40 ids (class + 1,
    0 = unknown) or None, rgb [V,3] f32 in [0,1] or None."""
    if isinstance(src, (str, os.PathLike)):
        m = read_ply(src)
        labels = m.get("labels")
        rgb = m.get("rgb")
        rgb = None if rgb is None else rgb.astype(np.float32) / np.float32(255.0)
    else:
        m = src
        labels = None if m.get("labels") is None else np.asarray(m["labels"]) + 1
        rgb = None if m.get("rgb") is None else np.asarray(m["rgb"], np.float32)
    verts = np.asarray(m["verts"], np.float32)
    if pose_frame:
        verts = pose_frame_to_ngp(verts, one_m_to_scene_uom)
    if "faces" not in m:
        raise ValueError("the mesh has no faces")
    return {"verts": np.ascontiguousarray(verts, np.float32),
            "faces": np.ascontiguousarray(m["faces"], np.int32),
            "labels": None if labels is None else np.asarray(labels).astype(np.int32),
            "rgb": rgb}


def read_frames(scene_root, exp_name=None, novel=False):
    """-> dict: stems [N] (output file names), poses [N,4,4] f32 (NGP frame),
    intrinsics (fx, fy, cx, cy), H, W, one_m_to_scene_uom."""
    with open(os.path.join(scene_root, "transforms_train.json")) as f:
        info = json.load(f)
    if novel:
        if exp_name is None:
            raise ValueError("novel viewpoints live under <scene>/<exp_name>/novel_viewpoints")
        with open(os.path.join(scene_root, exp_name, "novel_viewpoints",
                               "interpolated_data.json")) as f:
            frames = json.load(f)["frames"]
        stems = [os.path.splitext(os.path.basename(fr["nerf_label"]))[0] for fr in frames]
        mats = [fr["pose"] for fr in frames]
    else:
        frames = info["frames"]
        stems = [os.path.splitext(os.path.basename(fr["file_path"]))[0] for fr in frames]
        mats = [fr["transform_matrix"] for fr in frames]
    poses = np.stack([nerf_matrix_to_ngp(np.asarray(m, np.float32)) for m in mats]) \
        if mats else np.zeros((0, 4, 4), np.float32)
    return {"stems": stems, "poses": poses.astype(np.float32),
            "intrinsics": (float(info["fl_x"]), float(info["fl_y"]), float(info["cx"]),
                           float(info["cy"])),
            "H": int(info["h"]), "W": int(info["w"]),
            "one_m_to_scene_uom": float(info["one_m_to_scene_uom"])}


def render_views(mesh, poses, intrinsics, H, W, near, batch=16, device="cuda"):
    """Yields (first view index, ``ops.rasterize_mesh`` dict of device tensors)
    for the views in batches of ``batch``; the mesh is copied to the device once."""
    dev = torch.device(device)
    verts = torch.from_numpy(mesh["verts"]).to(dev)
    faces = torch.from_numpy(mesh["faces"]).to(dev)
    labels = None if mesh.get("labels") is None else torch.from_numpy(mesh["labels"]).to(dev)
    rgb = None if mesh.get("rgb") is None else torch.from_numpy(mesh["rgb"]).to(dev)
    poses = torch.as_tensor(np.asarray(poses, np.float32))
    for a in range(0, poses.shape[0], batch):
        p = poses[a:a + batch].to(dev)
        yield a, ops.rasterize_mesh(verts, faces, p, intrinsics, H, W, near,
                                    vertex_labels=labels, vertex_rgb=rgb)


def score_label_maps(pred, mesh_label, C=40):
    """2D score of NYU40 label maps (class + 1, 0 = unknown; numpy or tensors of
    any matching shape) against mesh-rendered ones, through ``SemanticsMeter``.
    Pixels whose mesh label is 0 or above C are ignored, as
    ``evaluate_semantic_mesh`` ignores such vertices; a prediction of 0 or
    above C counts as wrong.  -> {"mIoU", "total_acc", "mean_acc", "pixels"}."""
    p = torch.as_tensor(np.asarray(pred)).reshape(-1).to(torch.int64)
    t = torch.as_tensor(np.asarray(mesh_label)).reshape(-1).to(torch.int64)
    valid = (t >= 1) & (t <= C)
    truth = torch.where(valid, t - 1, torch.full_like(t, -1))
    # a prediction outside 1..C is a miss: give it a class the truth never is
    # when there is one; else it stays out of the matrix
    pr = torch.where((p >= 1) & (p <= C), p - 1, torch.full_like(p, -1))
    meter = SemanticsMeter(C)
    bad = (pr < 0) & valid
    if bool(bad.any()):
        pr = torch.where(bad, (truth + 1) % C, pr)
    meter.update(pr.numpy(), truth.numpy())
    if meter.conf_mat is None or not meter.conf_mat.any():
        return {"mIoU": float("nan"), "total_acc": float("nan"),
                "mean_acc": float("nan"), "pixels": 0}
    miou, total_acc, mean_acc = meter.measure()
    return {"mIoU": float(miou), "total_acc": float(total_acc), "mean_acc": float(mean_acc),
            "pixels": int(valid.sum())}
