"""Wall time of the mesh rasterizer (a record, not a gate): the analytic room's
labelled mesh at several grid steps and the bench field's exported mesh,
rendered into B views at H x W (``ops.rasterize_mesh``: both passes and the
read-back between them); one JSON line.  Host clock around synchronised,
warmed calls, the best of ``--reps``.

    python tools/mesh_raster_time.py [--steps 0.02 0.05 1.0] [--B 16] [--H 480 --W 640]
        [--no_field]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def _record(verts, faces, labels, poses, intr, H, W, near, reps):
    from ucsa_neural_rendering_amd import ops
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).cuda()
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32)).cuda()
    lab = torch.from_numpy(np.asarray(labels, np.int32)).cuda()
    p = torch.from_numpy(np.asarray(poses, np.float32)).cuda()
    out = ops.rasterize_mesh(v, f, p, intr, H, W, near, vertex_labels=lab)
    t = _time(lambda: ops.rasterize_mesh(v, f, p, intr, H, W, near, vertex_labels=lab), reps)
    B = p.shape[0]
    return {"F": int(f.shape[0]), "B": B, "ms_total": round(1e3 * t, 4),
            "ms_per_view": round(1e3 * t / B, 4),
            "covered": round(float((out["tri_id"] >= 0).float().mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.02, 0.05, 1.0])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no_field", action="store_true")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, \
        _slerp_loop_poses
    H, W = a.H, a.W
    intr = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    poses = _slerp_loop_poses(a.B, seed=123).numpy()
    room = SyntheticRoom(0)
    rec = {"H": H, "W": W, "B": a.B}
    for s in a.steps:
        m = room.labelled_mesh(s)
        rec[f"room_{s}"] = _record(m["verts"], m["faces"], m["labels"], poses, intr, H, W,
                                   0.05, a.reps)
    if not a.no_field:
        from tools.bench_legs.common import build_field
        net, _ = build_field("cuda", train_steps=200)
        aabb = [-3.05, -3.05, -3.05, 3.05, 3.05, 3.05]
        m = net.extract_semantic_mesh(256, 0.5, aabb)
        rec["bench_field_256"] = _record(m["verts"], m["faces"], m["labels"] + 1, poses, intr,
                                         H, W, 0.05, a.reps)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
