"""Device time of the nearest-point-on-a-surface search (a record, not a gate):
what the grid of faces costs next to the nearest-vertex search on the same
sets, what sorting the queries by cell is worth, how much the cell size
matters, and what a chunked torch brute force of the same formula takes.

Queries: the vertices of the analytic room's mesh at step 0.05 and 0.02;
targets: the room's meshes at step 1.0 (466 faces), 0.25 and 0.05; ``max_dist``
0.5:

  hip sorted     ops.nearest_triangle on the grid of ops.triangle_grid (default
                 cell), queries handed over in cell order.  The whole call: the
                 queries' key kernel and torch's stable sort are in it;
  hip unsorted   the same with sort_queries=False: the search kernel alone, the
                 queries in the mesh's own vertex order;
  hip cell x     sorted, with the cell at 1/4 and 4 times the default (a cell
                 that the caps on cells and pairs raise is printed as it ended);
  grid           ops.triangle_grid itself (counts, scan, pairs, sort, packing,
                 with the host reads that shape the grid);
  vertex         ops.nearest_point of the same queries against the target's
                 vertices on the grid of ops.point_grid: the search this one
                 stands next to;
  torch          the definition's formula in torch over chunks of queries sized
                 to --pair_budget pairs, on the first --torch_queries queries
                 (fewer where the target has many faces: at most 16 chunks).

Before anything is timed all hip variants must give the same face, dist2 and
bary bytes, and torch's dist2 must agree with the kernel's where both match
(the same float32 expressions, so the share of equal bytes is printed; a
difference above 1e-3 relative + 1e-8 absolute is an error, which leaves room
for a division that torch rounds differently on a dist2 next to 0).  All variants alternate in one process;
device events after a warm-up; median / best / worst ms.  One JSON line, then a
table, both also written to --out.

    python tools/surface_time.py [--query_steps 0.05 0.02] [--target_steps 1.0 0.25 0.05]
        [--max_dist 0.5] [--rounds 7] [--pair_budget 4194304] [--torch_queries 65536]
        [--out profiles/surface_time.txt] [--commit ID] [--parent ID]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.nearest_time import _time  # noqa: E402


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def torch_closest(A, B, C, q):
    """dist2 [Q,F] of the definition (include/ucsa_hip.h), every step a float32 torch op"""
    a, b, c = ([X[None, :, k] - q[:, None, k] for k in range(3)] for X in (A, B, C))
    ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
    na, nb, nc = [-x for x in a], [-x for x in b], [-x for x in c]
    d1, d2, d3, d4, d5, d6 = _dot(ab, na), _dot(ac, na), _dot(ab, nb), _dot(ac, nb), _dot(ab, nc), \
        _dot(ac, nc)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    den = one / ((va + vb) + vc)
    v, w = vb * den, vc * den
    v = torch.where(v < 0, zero, v)
    v = torch.where(v > 1, one, v)
    t = one - v
    w = torch.where(w < 0, zero, w)
    w = torch.where(w > t, t, w)
    wb = e43 / (e43 + e56)
    for cond, cv, cw in reversed((((d1 <= 0) & (d2 <= 0), zero, zero),
                                  ((d3 >= 0) & (d4 <= d3), one, zero),
                                  ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                                  ((d6 >= 0) & (d5 <= d6), zero, one),
                                  ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                                  ((va <= 0) & (e43 >= 0) & (e56 >= 0), one - wb, wb))):
        v, w = torch.where(cond, cv, v), torch.where(cond, cw, w)
    p = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
    return (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]


def torch_brute(V, Fc, Q, max_dist, pair_budget):
    A, B, C = (V[Fc[:, k].long()] for k in range(3))
    step = max(1, pair_budget // max(int(Fc.shape[0]), 1))
    best = []
    for s in range(0, Q.shape[0], step):
        d2 = torch_closest(A, B, C, Q[s:s + step])
        best.append(torch.nan_to_num(d2, nan=float("inf")).min(1).values)
    d2 = torch.cat(best)
    return torch.where(d2 <= max_dist * max_dist, d2, torch.full_like(d2, float("inf")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--query_steps", type=float, nargs="+", default=[0.05, 0.02])
    ap.add_argument("--target_steps", type=float, nargs="+", default=[1.0, 0.25, 0.05])
    ap.add_argument("--max_dist", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pair_budget", type=int, default=1 << 22)
    ap.add_argument("--torch_queries", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_time.txt"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    dev, md = "cuda", a.max_dist
    room = SyntheticRoom(0)
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "max_dist": md, "cases": {}}
    same = lambda x, y: all(torch.equal(p.view(torch.int32), q.view(torch.int32))
                            for p, q in zip(x, y))
    targets = {ts: room.labelled_mesh(ts) for ts in a.target_steps}
    for qs in a.query_steps:
        Q = torch.from_numpy(np.asarray(room.labelled_mesh(qs)["verts"], np.float32)).to(dev)
        for ts, m in targets.items():
            V = torch.from_numpy(np.asarray(m["verts"], np.float32)).to(dev)
            Fc = torch.from_numpy(np.asarray(m["faces"], np.int32)).to(dev)
            base = ops.triangle_grid(V, Fc)
            grids = {f"hip cell x{k:g}": ops.triangle_grid(V, Fc, base["cell"] * k)
                     for k in (0.25, 4.0)}
            pg = ops.point_grid(V)
            fns = {"hip sorted": lambda: ops.nearest_triangle(base, Q, md),
                   "hip unsorted": lambda: ops.nearest_triangle(base, Q, md, sort_queries=False)}
            for k, g in grids.items():
                fns[k] = lambda g=g: ops.nearest_triangle(g, Q, md)
            want = fns["hip sorted"]()
            for k, fn in fns.items():
                assert same(fn(), want), k
            nt = max(1, min(a.torch_queries, int(Q.shape[0]),
                            16 * max(1, a.pair_budget // int(Fc.shape[0]))))
            Qt = Q[:nt].contiguous()
            td2 = torch_brute(V, Fc, Qt, md, a.pair_budget)
            wd2 = want[1][:nt]
            both = torch.isfinite(td2) & torch.isfinite(wd2)
            assert float((torch.isfinite(td2) != torch.isfinite(wd2)).float().mean()) < 1e-3, \
                "torch: other matches"
            assert torch.allclose(td2[both], wd2[both], rtol=1e-3, atol=1e-8), "torch: dist2"
            equal = float((td2.view(torch.int32) == wd2.view(torch.int32)).float().mean())
            vi, vd2 = ops.nearest_point(pg, Q, md)
            hit = want[0] >= 0
            case = {"queries": int(Q.shape[0]), "faces": int(Fc.shape[0]), "verts": int(V.shape[0]),
                    "cell": base["cell"], "dims": list(base["dims"]), "pairs": base["n_pairs"],
                    "cells": {k: [g["cell"], g["n_pairs"]] for k, g in grids.items()},
                    "matched": round(float(hit.float().mean()), 5),
                    "mean_dist": round(float(want[1][hit].double().sqrt().mean()), 5),
                    "vertex_matched": round(float((vi >= 0).float().mean()), 5),
                    "vertex_mean_dist": round(float(vd2[vi >= 0].double().sqrt().mean()), 5),
                    "torch_queries": nt, "torch_equal_bytes": round(equal, 5)}
            fns["grid"] = lambda: ops.triangle_grid(V, Fc)
            fns["vertex"] = lambda: ops.nearest_point(pg, Q, md)
            fns["torch"] = lambda: torch_brute(V, Fc, Qt, md, a.pair_budget)
            case.update(_time(fns, a.rounds))
            rec["cases"][f"queries {qs:g}, target {ts:g}"] = case
    out = [json.dumps(rec), "",
           f"nearest point on a surface, ms per call (median / best / worst of {a.rounds} alternated "
           f"rounds), max_dist {md:g}; commit {a.commit} (parent {a.parent}), {rec['device']}",
           "hip sorted / hip cell x: the whole call, with the queries' keys and their sort; hip "
           "unsorted: the search kernel alone; grid: with the host reads that shape it; vertex: "
           "ops.nearest_point against the target's vertices; torch: on the first torch_queries "
           "queries only"]
    for name, c in rec["cases"].items():
        out.append(f"{name}: {c['queries']} queries, {c['faces']} faces, cell {c['cell']:.4f}, dims "
                   f"{c['dims']}, {c['pairs']} pairs; matched {c['matched']} at mean distance "
                   f"{c['mean_dist']} (vertex: {c['vertex_matched']} at {c['vertex_mean_dist']}); "
                   f"torch on {c['torch_queries']} queries, {c['torch_equal_bytes']} of dist2 "
                   "equal to the bit")
        for k, v in c.items():
            if isinstance(v, dict) and "median_ms" in v:
                extra = f"   (cell {c['cells'][k][0]:.4f}, {c['cells'][k][1]} pairs)" \
                    if k in c["cells"] else ""
                out.append(f"    {k:<16} {v['median_ms']:.4f} / {v['best']:.4f} / {v['worst']:.4f}"
                           + extra)
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
