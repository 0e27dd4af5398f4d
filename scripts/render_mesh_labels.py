#!/usr/bin/env python3
"""Render a labelled mesh into a scene's posed frames (GPU rasterizer,
``ops.rasterize_mesh``): per frame ``mesh_label/<stem>.png`` (uint8 NYU40 id,
0 = nothing / unknown), ``mesh_depth/<stem>.png`` (uint16 millimetres, 0 =
nothing; the layout of ``depth/``) and, when the mesh has colours,
``mesh_image/<stem>.png``.  With ``--score``, the predict pass's
``nerf_label`` (and ``seg_label``) PNGs of the same frames are scored against
the mesh labels (2D mIoU / accuracy) and one JSON line is printed.

    python scripts/render_mesh_labels.py --scene_root <root>/<scene> --mesh M.ply \\
        [--pose_frame] [--exp_name E] [--novel_viewpoints] [--near 0.05] \\
        [--out_dir D] [--score]

The mesh is read in the field's (NGP) frame, or with ``--pose_frame`` in the
frame of the transforms JSON's poses in metres (what
``scripts/export_semantic_mesh.py --one_m_to_scene_uom`` writes; the scale is
the JSON's ``one_m_to_scene_uom``).  Frames: those of transforms_train.json, or
with ``--novel_viewpoints`` those of ``<exp>/novel_viewpoints/
interpolated_data.json``.  Output directory: ``--out_dir``, else
``<scene>/<exp>[/novel_viewpoints]`` with ``--exp_name``, else the scene root."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ucsa_neural_rendering_amd.utils.mesh_render import (  # noqa: E402
    load_mesh, read_frames, render_views, score_label_maps)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--scene_root", required=True, help="<root>/<scene>")
    p.add_argument("--mesh", required=True, help="labelled mesh (.ply)")
    p.add_argument("--pose_frame", action="store_true",
                   help="the mesh is in the JSON pose frame, in metres")
    p.add_argument("--exp_name", default=None)
    p.add_argument("--novel_viewpoints", action="store_true")
    p.add_argument("--near", type=float, default=0.05, help="near plane, scene units")
    p.add_argument("--out_dir", default=None)
    p.add_argument("--score", action="store_true")
    p.add_argument("--num_classes", type=int, default=40)
    p.add_argument("--batch", type=int, default=16, help="views per rasterizer call")
    return p.parse_args(argv)


def main(argv=None):
    from PIL import Image
    a = parse_args(argv)
    if a.score and a.exp_name is None:
        raise SystemExit("--score reads <scene>/<exp_name>/...: give --exp_name")
    fr = read_frames(a.scene_root, a.exp_name, a.novel_viewpoints)
    uom = fr["one_m_to_scene_uom"]
    mesh = load_mesh(a.mesh, pose_frame=a.pose_frame, one_m_to_scene_uom=uom)
    sub = os.path.join(a.exp_name, "novel_viewpoints" if a.novel_viewpoints else "") \
        if a.exp_name else ""
    out_dir = a.out_dir or os.path.join(a.scene_root, sub)
    kinds = ["mesh_label", "mesh_depth"] + (["mesh_image"] if mesh["rgb"] is not None else [])
    for k in kinds:
        os.makedirs(os.path.join(out_dir, k), exist_ok=True)
    t_render, labels = 0.0, {}
    stems = fr["stems"]
    it = render_views(mesh, fr["poses"], fr["intrinsics"], fr["H"], fr["W"], a.near, a.batch)
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            start, out = next(it)
        except StopIteration:
            break
        torch.cuda.synchronize()
        t_render += time.perf_counter() - t0
        lab = out["label"].clamp(0, 255).to(torch.uint8).cpu().numpy()
        mm = torch.round(out["depth"].double() / uom * 1000.0).clamp(0, 65535)
        mm = mm.to(torch.int32).cpu().numpy().astype(np.uint16)
        img = None
        if "rgb" in out:
            img = torch.round(out["rgb"].clamp(0, 1) * 255.0).to(torch.uint8).cpu().numpy()
        for i in range(lab.shape[0]):
            stem = stems[start + i]
            Image.fromarray(lab[i]).save(os.path.join(out_dir, "mesh_label", stem + ".png"))
            Image.fromarray(mm[i]).save(os.path.join(out_dir, "mesh_depth", stem + ".png"))
            if img is not None:
                Image.fromarray(img[i]).save(os.path.join(out_dir, "mesh_image", stem + ".png"))
            labels[stem] = lab[i]
    n = len(stems)
    rec = {"out_dir": out_dir, "frames": n, "faces": int(mesh["faces"].shape[0]),
           "render_ms_per_view": round(1000.0 * t_render / max(n, 1), 3)}
    if a.score:
        src = os.path.join(a.scene_root, a.exp_name,
                           "novel_viewpoints" if a.novel_viewpoints else "")
        for name in ("nerf_label", "seg_label"):
            preds, truths = [], []
            for stem in stems:
                path = os.path.join(src, name, stem + ".png")
                if os.path.exists(path):
                    preds.append(np.asarray(Image.open(path)))
                    truths.append(labels[stem])
            if preds:
                rec[name] = score_label_maps(np.stack(preds), np.stack(truths), a.num_classes)
                rec[name]["frames"] = len(preds)
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
