"""Device time of the label-fusion accumulate (a record, not a gate): votes of B
views at H x W into the table of the analytic room's mesh at a fine and a coarse
grid step, with coherent predictions (the mesh's own clean label render) and
with uniformly random ones.  Three ways to the same table, alternated in one
process and timed with device events after a warm-up:

  hip      ops.fuse_label_votes (csrc/label_fusion.hip: lanes of a wave with an
           equal (vertex, class) are added up before one atomic);
  naive    the same kernel file's one-atomic-per-pixel form (a template flag);
  torch    what one would write without the kernel: flattened keys and
           ``index_add_`` into an int64 table on the same device (non-voting
           pixels add 0 to the unused cell 0, so there is no mask and no sync).

Each round times ``--inner`` back-to-back calls of one variant; ``--rounds``
rounds per variant, interleaved.  Per variant: the median per-view time and the
spread (min .. max over the rounds).  Next to them the rasterizer's time for the
same batch (``ops.rasterize_mesh`` with vertex ids, host clock, synchronised:
it reads a total back between its passes).  Every variant's table is checked
against the others before timing.  One JSON line, then a table.

    python tools/label_fusion_time.py [--steps 0.05 1.0] [--B 16] [--H 480 --W 640]
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

NC = 40


def _torch_votes(table, vid, pred):
    v = vid.reshape(-1).to(torch.int64)
    c = pred.reshape(-1).to(torch.int64)
    ok = (v >= 1) & (v <= table.shape[0]) & (c >= 1) & (c <= NC)
    key = torch.where(ok, (v - 1) * (NC + 1) + c, torch.zeros_like(v))
    table.view(-1).index_add_(0, key, ok.to(torch.int64))
    return table


def _rounds(fns, rounds, inner):
    """fns: name -> callable; -> name -> list of ms per call, one per round"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.05, 1.0])
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, \
        _slerp_loop_poses
    H, W, B = a.H, a.W, a.B
    intr = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    poses = _slerp_loop_poses(B, seed=123).cuda()
    room = SyntheticRoom(0)
    rec = {"H": H, "W": W, "B": B, "rounds": a.rounds, "inner": a.inner, "cases": {}}
    for s in a.steps:
        m = room.labelled_mesh(s)
        V = m["verts"].shape[0]
        v = torch.from_numpy(np.ascontiguousarray(m["verts"], np.float32)).cuda()
        f = torch.from_numpy(np.ascontiguousarray(m["faces"], np.int32)).cuda()
        ids = torch.arange(1, V + 1, dtype=torch.int32, device="cuda")
        raster = lambda: ops.rasterize_mesh(v, f, poses, intr, H, W, 0.05,  # noqa: E731
                                            vertex_labels=ids)
        vid = raster()["label"]
        raster_ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            raster()
            torch.cuda.synchronize()
            raster_ms.append(1e3 * (time.perf_counter() - t0) / B)
        clean = ops.rasterize_mesh(v, f, poses, intr, H, W, 0.05, vertex_labels=torch.from_numpy(
            np.asarray(m["labels"], np.int32)).cuda())["label"].to(torch.uint8)
        g = torch.Generator(device="cuda").manual_seed(0)
        rand = torch.randint(1, NC + 1, vid.shape, generator=g, device="cuda").to(torch.uint8)
        for pname, pred in (("coherent", clean), ("random", rand)):
            tabs = {k: torch.zeros(V, NC + 1, dtype=torch.int64, device="cuda")
                    for k in ("hip", "naive", "torch")}
            fns = {"hip": lambda: ops.fuse_label_votes(tabs["hip"], vid, pred),
                   "naive": lambda: ops.fuse_label_votes(tabs["naive"], vid, pred,
                                                         _one_atomic_per_pixel=True),
                   "torch": lambda: _torch_votes(tabs["torch"], vid, pred)}
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            assert torch.equal(tabs["hip"], tabs["naive"])
            assert torch.equal(tabs["hip"][:, 1:], tabs["torch"][:, 1:])
            ms = _rounds(fns, a.rounds, a.inner)
            case = {"V": V, "F": int(f.shape[0]),
                    "votes_per_view": int(tabs["hip"].sum().item() // (B * (1 + 1 + a.rounds *
                                                                            a.inner))),
                    "raster_ms_per_view": round(float(np.median(raster_ms)), 4)}
            for k, xs in ms.items():
                xs = np.asarray(xs) / B
                case[k] = {"median_ms_per_view": round(float(np.median(xs)), 5),
                           "min": round(float(xs.min()), 5), "max": round(float(xs.max()), 5)}
            rec["cases"][f"room_{s}_{pname}"] = case
    print(json.dumps(rec))
    print(f"\naccumulate, ms per {W}x{H} view (median [min .. max] of {a.rounds} rounds x "
          f"{a.inner} calls of {B} views)")
    for name, c in rec["cases"].items():
        cols = "  ".join(f"{k} {c[k]['median_ms_per_view']:.5f} [{c[k]['min']:.5f} .. "
                         f"{c[k]['max']:.5f}]" for k in ("hip", "naive", "torch"))
        print(f"{name:>22} V={c['V']:<7} {cols}  rasterize {c['raster_ms_per_view']:.4f}")


if __name__ == "__main__":
    main()
