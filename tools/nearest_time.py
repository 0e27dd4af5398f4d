"""Device time of the nearest-point search (a record, not a gate), so that the
next reader knows what the cell grid buys over a chunked torch ``cdist``, what
sorting the queries by cell is worth, and how much the cell size matters -- the
numbers a wave-cooperative form of the kernel would have to beat.

Points: the analytic room's mesh at step 0.05 and 0.02; queries: the same
vertices shifted by half a step along x; ``max_dist`` 0.05 and 0.5:

  hip sorted     ops.nearest_point on the grid of ops.point_grid (default cell),
                 queries handed over in cell order.  The time is the whole call:
                 the queries' key kernel and torch's stable sort of the keys
                 are in it, next to the search kernel;
  hip unsorted   the same with sort_queries=False: the search kernel alone, the
                 queries in the mesh's own vertex order;
  hip presorted  sort_queries=False on queries permuted into cell order
                 beforehand: the search kernel alone on coherent waves;
  hip cell x     sorted, with the cell at 0.5, 1 and 2 times the default;
  grid           ops.point_grid itself (keys, sort, offsets, packing).  The call
                 reads the points' box back to the host (two .tolist()) to
                 shape the grid, so this time holds a host round trip;
  torch cdist    cdist + min over chunks of queries sized to --pair_budget
                 pairs, cdist's default mode (|q|^2 + |p|^2 - 2 q.p through a
                 matrix product), on the first --torch_queries queries only
                 (the whole 0.02 mesh is 3.3e11 pairs);
  torch broadcast  the differences themselves, (q - p)^2 summed and min over
                 chunks a quarter as large: the definition's arithmetic in torch,
                 on the same queries.

Before anything is timed all hip variants must give the same index and dist2
bytes.  Against torch, dist2 is compared, not the indices (torch's ties are its
own), with bounds from the arithmetic: float32 d2 is within 6 ulp of the true
squared distance and so is the broadcast form, whatever the order of its sum, so
the two must agree to 16 ulp (2^-20) relative; cdist's default form errs by the rounding of the squared norms it
subtracts, so it must agree to 16 ulp of |q|^2 + max |p|^2, absolute (about 1e-3
of a dist2 of 0.025^2 in a room 6 wide).  A query may match on one side only
where dist2 is within the bound of the radius.  All variants, torch included,
alternate in one process; device events after a warm-up; median / best / worst
ms.  One JSON line, then a table.

    python tools/nearest_time.py [--steps 0.05 0.02] [--max_dists 0.05 0.5] [--rounds 7]
        [--pair_budget 268435456] [--torch_queries 65536] [--commit ID] [--parent ID]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


U = 2.0 ** -24


def _gather(parts, max_dist):
    d2, idx = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    hit = d2 <= max_dist * max_dist
    return torch.where(hit, idx, torch.full_like(idx, -1)), d2


def torch_cdist(points, queries, max_dist, pair_budget):
    """cdist's default mode: |q|^2 + |p|^2 - 2 q.p through a matrix product"""
    step = max(1, pair_budget // max(points.shape[0], 1))
    parts = []
    for a in range(0, queries.shape[0], step):
        d, j = torch.cdist(queries[a:a + step], points).min(1)
        parts.append((d * d, j))
    return _gather(parts, max_dist)


def torch_broadcast(points, queries, max_dist, pair_budget):
    """the differences themselves: the definition's arithmetic in torch"""
    step = max(1, pair_budget // (4 * max(points.shape[0], 1)))
    parts = []
    for a in range(0, queries.shape[0], step):
        parts.append((queries[a:a + step, None, :] - points[None, :, :]).square().sum(-1).min(1))
    return _gather(parts, max_dist)


def differs_from_torch(index, dist2, t_index, t_dist2, tol, max_dist):
    """every query: the same dist2 to ``tol`` (a tensor, absolute); matched on one
    side only where dist2 is within ``tol`` of the radius -> None, or what differs"""
    lim2 = max_dist * max_dist
    hit, thit = index >= 0, t_index >= 0
    near = (t_dist2 - dist2).abs() <= tol
    ok = (hit & near) | (~hit & ~thit) | (~hit & thit & (t_dist2 >= lim2 - tol))
    if bool(ok.all()):
        return None
    off = ((t_dist2 - dist2).abs() / tol)[hit]
    return (f"{int((~ok).sum())} of {ok.numel()} queries differ from torch: matched "
            f"{int(hit.sum())} against {int(thit.sum())}, dist2 off by up to "
            f"{float(off.max()) if off.numel() else 0.0:.3g} times the bound")


def _time(fns, rounds):
    """alternated: every round runs every variant once, in the same order"""
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
    return {k: {"median_ms": round(float(np.median(v)), 4), "best": round(float(np.min(v)), 4),
                "worst": round(float(np.max(v)), 4)} for k, v in out.items()}


def sorted_order(ops, grid, Q, keys):
    """the order in which ops.nearest_point hands sorted queries to the kernel"""
    import ctypes as C
    from ucsa_neural_rendering_amd import _lib
    rc = _lib.lib().ucsa_point_cell_keys(C.c_void_p(Q.data_ptr()), Q.shape[0],
                                         (C.c_float * 3)(*grid["origin"]), grid["cell"],
                                         (C.c_uint32 * 3)(*grid["dims"]), 0,
                                         C.c_void_p(keys.data_ptr()), None)
    assert rc == 0, rc
    return torch.sort(keys, stable=True).indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.05, 0.02])
    ap.add_argument("--max_dists", type=float, nargs="+", default=[0.05, 0.5])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pair_budget", type=int, default=1 << 28)
    ap.add_argument("--torch_queries", type=int, default=65536)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    dev = "cuda"
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "cases": {}}
    for step in a.steps:
        verts = np.asarray(SyntheticRoom(0).labelled_mesh(step)["verts"], np.float32)
        P = torch.from_numpy(verts).to(dev)
        Q = (P + torch.tensor([0.5 * step, 0.0, 0.0], device=dev)).contiguous()
        base = ops.point_grid(P)
        grids = {f"hip cell x{m:g}": ops.point_grid(P, base["cell"] * m) for m in (0.5, 1.0, 2.0)}
        for md in a.max_dists:
            fns = {"hip sorted": lambda md=md: ops.nearest_point(base, Q, md),
                   "hip unsorted": lambda md=md: ops.nearest_point(base, Q, md, sort_queries=False)}
            for k, g in grids.items():
                fns[k] = lambda g=g, md=md: ops.nearest_point(g, Q, md)
            want = fns["hip sorted"]()
            for k, fn in fns.items():
                got = fn()
                assert torch.equal(got[0], want[0]) and torch.equal(
                    got[1].view(torch.int32), want[1].view(torch.int32)), k
            keys = torch.empty(Q.shape[0], dtype=torch.int32, device=dev)
            perm = sorted_order(ops, base, Q, keys)
            Qs = Q[perm].contiguous()
            fns["hip presorted"] = lambda md=md: ops.nearest_point(base, Qs, md, sort_queries=False)
            got = fns["hip presorted"]()
            assert torch.equal(got[0], want[0][perm]) and torch.equal(
                got[1].view(torch.int32), want[1][perm].view(torch.int32)), "hip presorted"
            nt = min(a.torch_queries, int(Q.shape[0]))
            Qt = Q[:nt].contiguous()
            wi, wd2 = want[0][:nt], want[1][:nt]
            # float32 d2 is within 6 ulp of the true squared distance, the broadcast form
            # likewise: 16 ulp relative between them.  cdist's default form errs by the
            # rounding of the squared norms it subtracts: 16 ulp of |q|^2 + max |p|^2, absolute
            bi, bd2 = torch_broadcast(P, Qt, md, a.pair_budget)
            bad = differs_from_torch(wi, wd2, bi, bd2, 16 * U * torch.minimum(wd2, bd2), md)
            assert bad is None, "broadcast: " + bad
            ci, cd2 = torch_cdist(P, Qt, md, a.pair_budget)
            norms = Qt.square().sum(1) + float(P.square().sum(1).max())
            bad = differs_from_torch(wi, wd2, ci, cd2, 16 * U * norms, md)
            assert bad is None, "cdist: " + bad
            both = (wi >= 0) & (wd2 > 0)
            mm_dev = float(((cd2 - wd2).abs() / wd2)[both].max()) if bool(both.any()) else 0.0
            hit = want[0] >= 0
            case = {"points": int(P.shape[0]), "cell": base["cell"], "dims": list(base["dims"]),
                    "matched": round(float(hit.float().mean()), 4), "torch_queries": nt,
                    "cdist_worst_rel_dist2_deviation": mm_dev}
            fns["grid"] = lambda: ops.point_grid(P)
            fns["torch cdist"] = lambda md=md: torch_cdist(P, Qt, md, a.pair_budget)
            fns["torch broadcast"] = lambda md=md: torch_broadcast(P, Qt, md, a.pair_budget)
            case.update(_time(fns, a.rounds))
            rec["cases"][f"step {step:g}, max_dist {md:g}"] = case
    print(json.dumps(rec))
    print(f"\nnearest point, ms per call (median / best / worst of {a.rounds} alternated rounds); "
          f"commit {a.commit} (parent {a.parent}), {rec['device']}")
    print("hip sorted / hip cell x: the whole call, with the queries' keys and their sort; hip "
          "unsorted / presorted: the search kernel alone; grid: with a host read-back of the box; "
          "torch cdist / broadcast: on the first torch_queries queries only")
    for name, c in rec["cases"].items():
        print(f"{name}: {c['points']} points and queries, cell {c['cell']:.4f}, dims {c['dims']}, "
              f"matched {c['matched']}; torch on {c['torch_queries']} queries, cdist's dist2 "
              f"off by up to {c['cdist_worst_rel_dist2_deviation']:.3g} relative")
        for k, v in c.items():
            if isinstance(v, dict):
                print(f"    {k:<16} {v['median_ms']:.4f} / {v['best']:.4f} / {v['worst']:.4f}")


if __name__ == "__main__":
    main()
