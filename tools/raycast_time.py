"""Device time of the ray cast against a mesh (a record, not a gate).

One 480 x 640 view of the analytic room's meshes (SyntheticRoom(0).labelled_mesh at
the given steps) from a camera of the loop inside the room:

  cast      ucsa_raycast_mesh alone: rays and grid prepared, rays in pixel order
  sorted    the same with sort_rays=True (the entry-cell sort included)
  occluded  ucsa_mesh_occluded on the same rays
  views     utils.mesh_raycast.raycast_views: rays, cast, depth, labels
  raster    ops.rasterize_mesh for the same view
  brute     a chunked torch brute force of the same formula (float64 edge
            functions) on every ``--brute_stride``-th ray, scaled by the stride
  cell/4, cell*4   ``cast`` over grids with the cell a quarter of and four times
            the default
  visible   utils.mesh_raycast.visible_points: about 10^5 surface samples of the mesh
            x 16 views at 480 x 640

Alternated in one process, device events, after a warm-up; median / best.

    python tools/raycast_time.py [--steps 1.0 0.25 0.05] [--rounds 5] [--brute_stride 64]
        [--commit ID]
One JSON line, then a table."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640


def time_fns(fns, rounds):
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: {"median_ms": round(float(np.median(v)), 4), "best_ms": round(float(np.min(v)), 4)}
            for k, v in out.items()}


def brute_force(o, d, A, B, C, chunk_pairs=1 << 22):
    """the nearest hit of every ray among all faces: the contract's formula
    without its box clause, torch, float64 edge functions"""
    n = o.shape[0]
    best = torch.full((n,), float("inf"), device=o.device)
    kz = d.abs().argmax(1)
    perm = torch.stack([(kz + 1) % 3, (kz + 2) % 3, kz], 1)               # kx, ky, kz
    op, dp = o.gather(1, perm), d.gather(1, perm)
    Sx, Sy = dp[:, 0] / dp[:, 2], dp[:, 1] / dp[:, 2]
    step = max(1, chunk_pairs // A.shape[0])
    for s in range(0, n, step):
        e = slice(s, s + step)
        idx = perm[e, None, :].expand(-1, A.shape[0], -1)
        XY = []
        for P in (A, B, C):
            q = P[None].expand(idx.shape[0], -1, -1).gather(2, idx) - op[e, None, :]
            XY.append(((q[..., 0] - Sx[e, None] * q[..., 2]).double(),
                       (q[..., 1] - Sy[e, None] * q[..., 2]).double(), q[..., 2].double()))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = XY
        U, V, Wt = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        det = U + V + Wt
        inside = (((U >= 0) & (V >= 0) & (Wt >= 0)) | ((U <= 0) & (V <= 0) & (Wt <= 0))) & (det != 0)
        t = ((U * Az + V * Bz + Wt * Cz) / det / dp[e, None, 2].double()).float()
        t = torch.where(inside & (t >= 0), t, torch.full_like(t, float("inf")))
        best[e] = t.min(1).values
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[1.0, 0.25, 0.05])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--brute_stride", type=int, default=64)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, _slerp_loop_poses
    from ucsa_neural_rendering_amd.utils.mesh_raycast import raycast_views, visible_points
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "view": [H, W], "brute_stride": a.brute_stride, "cases": {}}
    room = SyntheticRoom(0)
    poses = _slerp_loop_poses(16).cuda()
    K = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    o, d, nrm = ops.get_rays(poses[:1], K, H, W)
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    rc = ops.raycast
    for step in a.steps:
        m = room.labelled_mesh(step)
        mesh = {"verts": m["verts"].astype(np.float32), "faces": m["faces"].astype(np.int32),
                "labels": np.asarray(m["labels"], np.int32), "rgb": None}
        v, f = torch.from_numpy(mesh["verts"]).cuda(), torch.from_numpy(mesh["faces"]).cuda()
        lab = torch.from_numpy(mesh["labels"]).cuda()
        grid = ops.triangle_grid(v, f)
        fine, coarse = ops.triangle_grid(v, f, grid["cell"] / 4.0), ops.triangle_grid(v, f, grid["cell"] * 4.0)
        A, B, C = (v[f[:, k].long()] for k in range(3))
        ob, db = o[::a.brute_stride].contiguous(), d[::a.brute_stride].contiguous()
        area = ops.sample_mesh_surface(v, f, 1.0, 0, max_samples=1 << 31)["area"]
        dens = 1.0e5 / float(area.double().sum())
        pts = ops.sample_mesh_surface(v, f, dens, 0)["points"]
        fns = {"cast": lambda: rc.raycast_mesh(grid, o, d),
               "sorted": lambda: rc.raycast_mesh(grid, o, d, sort_rays=True),
               "occluded": lambda: rc.mesh_occluded(grid, o, d),
               "views": lambda: raycast_views(mesh, poses[:1], K, H, W, 0.05, 100.0, grid=grid),
               "raster": lambda: ops.rasterize_mesh(v, f, poses[:1], K, H, W, 0.05,
                                                    vertex_labels=lab),
               "brute": lambda: brute_force(ob, db, A, B, C),
               "cell/4": lambda: rc.raycast_mesh(fine, o, d),
               "cell*4": lambda: rc.raycast_mesh(coarse, o, d),
               "visible": lambda: visible_points(grid, pts, poses, K, H, W, 0.05, 100.0, 0.01)}
        case = {"faces": int(f.shape[0]), "pairs": grid["n_pairs"], "cell": round(grid["cell"], 5),
                "dims": list(grid["dims"]), "cells": [round(fine["cell"], 5), round(coarse["cell"], 5)],
                "samples": int(pts.shape[0]), **time_fns(fns, a.rounds)}
        case["brute_scaled_ms"] = round(case["brute"]["median_ms"] * o.shape[0] / ob.shape[0], 1)
        face, t, _ = rc.raycast_mesh(grid, o, d)
        tb = brute_force(ob, db, A, B, C)
        case["hit_share"] = round(float((face >= 0).float().mean()), 5)
        same = (t[::a.brute_stride] - tb).abs() <= 1e-4 * tb.abs().clamp_min(1.0)
        case["brute_agrees"] = round(float((same | (torch.isinf(tb) & torch.isinf(t[::a.brute_stride])))
                                           .float().mean()), 5)
        case["seen_share"] = round(float((visible_points(grid, pts, poses, K, H, W, 0.05, 100.0, 0.01)
                                          > 0).float().mean()), 5)
        rec["cases"][f"step {step}"] = case
        print(f"step {step}: done", file=sys.stderr, flush=True)
        del fns, grid, fine, coarse, A, B, C
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    print(f"\nray cast, one {H} x {W} view of the room meshes; ms median / best of {a.rounds}; commit "
          f"{a.commit}, {rec['device']}")
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, c in rec["cases"].items():
        print(f"{name} ({c['faces']} faces, {c['pairs']} pairs, cell {c['cell']}, dims {c['dims']}, "
              f"{c['hit_share']} of the rays hit)\n"
              f"  cast {fmt(c, 'cast')}   sorted rays {fmt(c, 'sorted')}   any hit {fmt(c, 'occluded')}   "
              f"raycast_views {fmt(c, 'views')}   rasterize_mesh {fmt(c, 'raster')}\n"
              f"  cell/4 ({c['cells'][0]}) {fmt(c, 'cell/4')}   cell*4 ({c['cells'][1]}) {fmt(c, 'cell*4')}   "
              f"torch brute force on 1/{a.brute_stride} of the rays {fmt(c, 'brute')} "
              f"(x {a.brute_stride} = {c['brute_scaled_ms']} ms; agrees on {c['brute_agrees']})\n"
              f"  visible_points, {c['samples']} samples x 16 views {fmt(c, 'visible')} "
              f"({c['seen_share']} seen by at least one)")


if __name__ == "__main__":
    main()
