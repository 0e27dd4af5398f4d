"""Device time of the fused ICP step (a record, not a gate).

Source points: the vertices of the analytic room's 0.05 mesh
(SyntheticRoom(0).labelled_mesh(0.05)) under a start transform 3 degrees and 0.05
away from the identity, which is the answer; in mesh order and in the cell order
of ``ops.register.cell_order``.  Targets: the room's meshes at the given steps.
``max_dist`` 0.5, mode "plane".

  fused     one ops.register.icp_sums call: transform, search, 29 sums
  nearest   ops.nearest_triangle alone on the already moved points (no sort inside)
  torch3    what the fused call replaces: a torch transform, ops.nearest_triangle,
            and float64 torch sums of the same 29 terms (closest point from the
            barycentric weights, r, J, the products, one sum each)
  loop      a whole utils.registration.register_points call from that start
            (grid and normals given, the sort and every 29-double read included)

Alternated in one process, device events, after a warm-up; median / best.

    python tools/register_time.py [--steps 1.0 0.25 0.05] [--rounds 5] [--commit ID]
        [--out profiles/register_time.txt]
One JSON line, then a table; both are also written to ``--out``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


def move(pts, T32):
    """R p + t, elementwise (a float32 matmul may run at reduced precision)"""
    return pts[:, 0:1] * T32[:, 0] + pts[:, 1:2] * T32[:, 1] + pts[:, 2:3] * T32[:, 2] + T32[:, 3]


def torch_sums(grid, v, f, unit, pts, T32, max_dist, ops):
    """the three-step form: the same terms, float64 torch sums (no fixed tree)"""
    q = move(pts, T32)
    face, _, bary = ops.nearest_triangle(grid, q.contiguous(), max_dist, sort_queries=False)
    hit = face >= 0
    fi = face.clamp_min(0).long()
    corners = v[f[fi].long()]                                         # [N,3,3]
    p = (corners * bary[:, :, None]).sum(1) - q
    n = unit[fi]
    r = (n * p).sum(1)
    J = torch.cat([torch.linalg.cross(q, n), n], 1).double()
    r = r.double()
    w = hit.double()
    cols = [(J[:, a] * J[:, b] * w).sum() for a, b in PAIRS] + \
        [(J[:, a] * r * w).sum() for a in range(6)] + [(r * r * w).sum(), w.sum()]
    return torch.stack(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[1.0, 0.25, 0.05])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_time.txt"))
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    from ucsa_neural_rendering_amd.utils import registration as REG
    room = SyntheticRoom(0)
    world = np.asarray(room.labelled_mesh(0.05)["verts"], np.float64)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    # the source is the fine mesh's vertices themselves and every launch is timed at the
    # loop's first transform, 3 degrees and 0.05 away from the answer (the identity)
    T = REG.compose(np.eye(4), np.concatenate([np.radians(3.0) * axis, [0.03, -0.03, 0.0265]]))
    src = torch.from_numpy(world.astype(np.float32)).cuda()
    T32 = torch.from_numpy(T[:3].astype(np.float32)).cuda()
    md = 0.5
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "points": int(src.shape[0]), "max_dist": md, "cases": {}}
    for step in a.steps:
        m = room.labelled_mesh(step)
        v = torch.from_numpy(np.asarray(m["verts"], np.float32)).cuda()
        f = torch.from_numpy(np.asarray(m["faces"], np.int32)).cuda()
        grid = ops.triangle_grid(v, f)
        unit = ops.register.face_unit_normals(v, f)
        srt = src[ops.register.cell_order(grid, src, T).long()].contiguous()
        q, qs = (move(p, T32) for p in (src, srt))
        q, qs = q.contiguous(), qs.contiguous()
        icp = ops.register.icp_sums
        fns = {"fused": lambda: icp(grid, v, f, unit, src, T, md),
               "fused sorted": lambda: icp(grid, v, f, unit, srt, T, md),
               "nearest": lambda: ops.nearest_triangle(grid, q, md, sort_queries=False),
               "nearest sorted": lambda: ops.nearest_triangle(grid, qs, md, sort_queries=False),
               "torch3": lambda: torch_sums(grid, v, f, unit, src, T32, md, ops),
               "torch3 sorted": lambda: torch_sums(grid, v, f, unit, srt, T32, md, ops),
               "loop": lambda: REG.register_points(src, v, f, init=T, max_dist=md, grid=grid)}
        case = {"faces": int(f.shape[0]), "pairs": grid["n_pairs"], "cell": round(grid["cell"], 5),
                **time_fns(fns, a.rounds)}
        out = REG.register_points(src, v, f, init=T, max_dist=md, grid=grid)
        s_f = icp(grid, v, f, unit, srt, T, md).cpu().numpy()
        s_t = torch_sums(grid, v, f, unit, srt, T32, md, ops).cpu().numpy()
        case.update(iterations=out["iterations"], converged=out["converged"], rank=out["rank"],
                    matched=out["matched"], rmse=out["rmse"],
                    first_rmse=out["history"][0]["rmse"], last_omega=out["history"][-1]["omega"],
                    last_upsilon=out["history"][-1]["upsilon"],
                    torch3_rel_diff=float(np.abs(s_f - s_t).max() / np.abs(s_f).max()))
        rec["cases"][f"step {step}"] = case
        print(f"step {step}: done", file=sys.stderr, flush=True)
        del fns, grid
        torch.cuda.empty_cache()
    lines = [json.dumps(rec), "",
             f"fused ICP step, {rec['points']} source points (the 0.05 room mesh's vertices, 3 deg / "
             f"0.05 off), max_dist {md}, mode plane; ms median / best of {a.rounds}; commit "
             f"{a.commit}, {rec['device']}"]
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, c in rec["cases"].items():
        lines.append(
            f"{name} ({c['faces']} faces, {c['pairs']} pairs, cell {c['cell']})\n"
            f"  mesh order:  fused {fmt(c, 'fused')}   nearest_triangle alone {fmt(c, 'nearest')}   "
            f"torch transform + nearest_triangle + float64 sums {fmt(c, 'torch3')}\n"
            f"  cell order:  fused {fmt(c, 'fused sorted')}   nearest_triangle alone "
            f"{fmt(c, 'nearest sorted')}   three-step {fmt(c, 'torch3 sorted')}\n"
            f"  register_points {fmt(c, 'loop')}: {c['iterations']} iterations, converged "
            f"{c['converged']}, rank {c['rank']}, matched {c['matched']}, rmse {c['first_rmse']:.3e} -> {c['rmse']:.3e}, last step "
            f"{c['last_omega']:.1e} rad / {c['last_upsilon']:.1e}; "
            f"fused and three-step sums agree to {c['torch3_rel_diff']:.1e} of the largest")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
