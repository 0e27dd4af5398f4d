"""Device time of the mesh-to-TSDF fill (a record, not a gate).

``ops.mesh_tsdf`` on the analytic room's meshes (SyntheticRoom(0).labelled_mesh at
the given steps) into n^3 lattices over [-3.05, 3.05]^3 with trunc = 4 voxels:

  kernel   ucsa_mesh_tsdf alone, grid and normals prepared
  whole    ops.mesh_tsdf building the triangle grid and the pseudonormals too
  queries  (a) the lattice materialised as a queries array, ops.signed_distance
           (the cell sort of the queries, ucsa_nearest_triangle, ucsa_mesh_sign)
           and the clamp and the masked write in torch: the same voxels
  brute    (b) what one would write without the kernel: torch, chunks of voxels
           against all faces, the closest point by Ericson's regions, unsigned;
           timed on every ``--brute_stride``-th lattice point per axis and
           scaled by stride^3 (the full lattice does not fit a sitting)

Alternated in one process, device events, after a warm-up; median / best.

    python tools/sdf_time.py [--steps 0.25 0.05] [--sizes 128 256] [--rounds 9]
        [--brute_stride 4] [--commit ID]
One JSON line, then a table."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI = -3.05, 3.05


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


def lattice(n, h, stride=1):
    ax = LO + torch.arange(0, n, stride, device="cuda", dtype=torch.float32) * h
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).contiguous()


def brute_force(pts, A, B, C, trunc, chunk_pairs=1 << 24):
    """unsigned distance of every point to the nearest of all faces within trunc"""
    out = torch.full((pts.shape[0],), float("inf"), device=pts.device)
    ab, ac = B - A, C - A
    step = max(1, chunk_pairs // A.shape[0])
    for s in range(0, pts.shape[0], step):
        p = pts[s:s + step, None, :]
        ap, bp, cp = p - A, p - B, p - C
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        den = 1.0 / (va + vb + vc)
        v, w = vb * den, vc * den                                     # the interior
        one, zero = torch.ones_like(v), torch.zeros_like(v)
        for cond, vv, ww in (
                ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0),
                 1 - (d4 - d3) / ((d4 - d3) + (d5 - d6)), (d4 - d3) / ((d4 - d3) + (d5 - d6))),
                ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                ((d6 >= 0) & (d5 <= d6), zero, one),
                ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                ((d3 >= 0) & (d4 <= d3), one, zero),
                ((d1 <= 0) & (d2 <= 0), zero, zero)):                 # the last that holds wins
            v, w = torch.where(cond, vv, v), torch.where(cond, ww, w)
        q = A + ab * v[..., None] + ac * w[..., None] - p
        out[s:s + step] = (q * q).sum(-1).min(1).values.sqrt()
    return torch.where(out <= trunc, out, torch.full_like(out, float("inf")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.25, 0.05])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--brute_stride", type=int, default=4)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "brute_stride": a.brute_stride, "cases": {}}
    room = SyntheticRoom(0)
    for step in a.steps:
        m = room.labelled_mesh(step)
        v = torch.from_numpy(m["verts"].astype(np.float32)).cuda()
        f = torch.from_numpy(m["faces"].astype(np.int32)).cuda()
        grid, normals = ops.triangle_grid(v, f), ops.mesh_pseudonormals(v, f)
        A, B, C = (v[f[:, k].long()] for k in range(3))
        for n in a.sizes:
            h = (HI - LO) / (n - 1)
            trunc = 4 * h
            vol = ops.tsdf_volume((n,) * 3, (LO,) * 3, h)
            pts = lattice(n, h)
            sub = lattice(n, h, a.brute_stride)

            def queries():
                sdf, face, _, _, _ = ops.signed_distance(grid, normals, v, f, pts, trunc)
                hit = face >= 0
                t = (sdf / trunc).clamp(-1.0, 1.0)
                vol["tsdf"].view(-1)[hit] = t[hit]
                vol["weight"].view(-1)[hit] = 1.0

            fns = {"kernel": lambda: ops.mesh_tsdf(vol, v, f, trunc, grid=grid, normals=normals),
                   "whole": lambda: ops.mesh_tsdf(vol, v, f, trunc), "queries": queries,
                   "brute": lambda: brute_force(sub, A, B, C, trunc)}
            case = {"faces": int(f.shape[0]), "pairs": grid["n_pairs"], "trunc": round(trunc, 5),
                    "band_share": None, **time_fns(fns, a.rounds)}
            case["band_share"] = round(float((vol["weight"] > 0).float().mean()), 5)
            scale = pts.shape[0] / sub.shape[0]
            case["brute_scaled_ms"] = round(case["brute"]["median_ms"] * scale, 2)
            rec["cases"][f"step {step}, {n}^3"] = case
            del vol, pts, sub, fns
            torch.cuda.empty_cache()
            print(f"step {step}, {n}^3: done", file=sys.stderr, flush=True)
    print(json.dumps(rec))
    print(f"\nmesh_tsdf, room meshes, trunc = 4 voxels; ms median / best of {a.rounds}; commit "
          f"{a.commit}, {rec['device']}")
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, c in rec["cases"].items():
        print(f"{name} ({c['faces']} faces, {c['pairs']} pairs, band {c['band_share']} of the "
              f"voxels)\n  kernel {fmt(c, 'kernel')}   whole {fmt(c, 'whole')}   queries array + "
              f"sign {fmt(c, 'queries')}   torch brute force on 1/{a.brute_stride}^3 of the lattice "
              f"{fmt(c, 'brute')} (x {a.brute_stride}^3 = {c['brute_scaled_ms']} ms)")


if __name__ == "__main__":
    main()
