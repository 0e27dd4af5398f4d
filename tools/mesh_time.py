"""Wall time of the labelled-mesh export on the bench field (a record, not a
gate): density lattice, marching cubes (both passes and the read-back), vertex
attributes, at each resolution; one JSON line.

    python tools/mesh_time.py [--res 256 512] [--train_steps 200] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn, reps):
    out, best = None, float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--train_steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.5)
    a = ap.parse_args()
    from tools.bench_legs.common import build_field
    from ucsa_neural_rendering_amd import ops
    net, _ = build_field("cuda", train_steps=a.train_steps)
    aabb = [-3.05, -3.05, -3.05, 3.05, 3.05, 3.05]
    rec = {"train_steps": a.train_steps, "aabb": aabb, "threshold": a.threshold}
    for r in a.res:
        sigma, t_lat = _timed(lambda: net.density_lattice(r, aabb), a.reps)
        _, lo, h = net._lattice_frame(r, aabb)
        (v, f, n), t_mc = _timed(lambda: ops.marching_cubes(sigma, a.threshold, lo.tolist(),
                                                            h.tolist()), a.reps)
        del sigma
        m, t_all = _timed(lambda: net.extract_semantic_mesh(r, a.threshold, aabb), 1)
        rec[str(r)] = {"lattice_s": t_lat, "marching_cubes_s": t_mc, "extract_total_s": t_all,
                       "V": int(v.shape[0]), "F": int(f.shape[0])}
        del v, f, n, m
        torch.cuda.empty_cache()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
