"""Device time of the soft label fusion (a record, not a gate): 16 views of the
analytic room at H x W, C = 40, against volumes of n^3 over [-3.05, 3.05]^3
(trunc = 4 voxels), and the mesh kernel on coherent and random vertex maps.
Alternated in one process and timed with device events after a warm-up; per
variant the median and the best ms per view.

  evidence hip B   ops.accumulate_voxel_evidence (csrc/voxel_map.hip), B views per call;
  vote hip B=16    ops.vote_voxel_labels on the argmax of the same beliefs: the hard
                   vote that the evidence path replaces;
  evidence torch   the same rule in plain torch: project, gather the rows, then
                   index_add_ into an int32 table [n, C+1] (no saturation, no
                   abstaining);
  mesh coherent    ops.fuse_label_evidence, one vertex per 32x32 pixel block;
  mesh random      the same with a random vertex per pixel;
  mesh hard ...    ops.fuse_label_votes on the same vertex maps (one class id per pixel).

One JSON line, then a table.

    python tools/evidence_time.py [--sizes 128 256] [--B 1 4 16] [--H 480 --W 640]
        [--commit ID] [--parent ID]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI = -3.05, 3.05
C = 40


def _torch_evidence(table, grid, depth, rows, P, intr, trunc):
    """one view in plain torch; table int32 [n, C+1], rows uint8 [H*W, C]"""
    fx, fy, cx, cy = intr
    H, W = depth.shape
    px, py, pz = grid
    d0, d1, d2 = px - P[0, 3], py - P[1, 3], pz - P[2, 3]
    c = [(d0 * P[0, r] + d1 * P[1, r]) + d2 * P[2, r] for r in range(3)]
    u = torch.floor((fx * c[0]) / c[2] + cx)
    v = torch.floor((fy * c[1]) / c[2] + cy)
    ok = (c[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    pix = torch.where(ok, v * W + u, torch.zeros_like(u)).long()
    z = depth.reshape(-1)[pix]
    sdf = z - c[2]
    ok &= torch.isfinite(z) & (z >= 1e-6) & (sdf >= -trunc) & (sdf <= trunc)
    vox = torch.nonzero(ok.reshape(-1)).squeeze(1)
    add = torch.ones(vox.shape[0], C + 1, dtype=torch.int32, device=table.device)
    add[:, 1:] = rows[pix.reshape(-1)[vox]]
    table.index_add_(0, vox, add)


def _time(fns, rounds):
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
    return out


def _stats(xs, per):
    xs = np.asarray(xs) / per
    return {"median_ms_per_view": round(float(np.median(xs)), 5),
            "best": round(float(xs.min()), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no_torch", action="store_true")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticSceneDataset
    H, W, N = a.H, a.W, a.views
    ds = SyntheticSceneDataset(0, N, H, W)
    intr = [float(v) for v in ds.intrinsics]
    depth = torch.stack([ds[i]["depth"].float() for i in range(N)]).contiguous()
    pred = torch.stack([(ds[i]["label"].long() + 1).clamp(0, 255).to(torch.uint8)
                        for i in range(N)]).contiguous()
    poses = ds.poses.float().contiguous()
    # beliefs: 0.9 on the frame's class, the rest spread evenly; no label: abstain
    p = torch.full((N, C, H, W), 0.1 / (C - 1), device="cuda")
    p.scatter_(1, (pred.long().clamp(1, C) - 1)[:, None], 0.9)
    scores = ops.log_evidence(p)
    scores[(pred == 0) | (pred > C)] = 0
    del p
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "H": H, "W": W, "C": C, "views": N, "rounds": a.rounds, "cases": {}, "mesh": {}}
    for n in a.sizes:
        h = (HI - LO) / (n - 1)
        trunc = 4 * h
        vol = ops.tsdf_volume((n, n, n), (LO,) * 3, h)
        tables = {f"evidence hip B={b}": ops.voxel_evidence(vol, C) for b in a.B}
        votes = ops.voxel_votes(vol, C)

        def soft(t, b):
            for s in range(0, N, b):
                ops.accumulate_voxel_evidence(t, vol, depth[s:s + b], scores[s:s + b],
                                              poses[s:s + b], intr, trunc)
        fns = {k: (lambda k=k, b=b: soft(tables[k], b)) for k, b in zip(tables, a.B)}
        fns["vote hip B=16"] = lambda: [ops.vote_voxel_labels(
            votes, vol, depth[s:s + 16], pred[s:s + 16], poses[s:s + 16], intr, trunc)
            for s in range(0, N, 16)]
        if not a.no_torch:
            ax = [LO + torch.arange(n, device="cuda", dtype=torch.float32) * h] * 3
            grid = (ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :])
            t32 = torch.zeros(n ** 3, C + 1, dtype=torch.int32, device="cuda")
            rows = scores.reshape(N, H * W, C)
            fns["evidence torch"] = lambda: [_torch_evidence(
                t32, grid, depth[i], rows[i], poses[i], intr, trunc) for i in range(N)]
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        first = tables[f"evidence hip B={a.B[0]}"]
        for k, t in tables.items():
            assert torch.equal(t.view(torch.int32), first.view(torch.int32)), k
        case = {"n": n, "evidence_MB": round((C + 1) * n ** 3 * 4 / 1e6, 1),
                "band_share": round(float((first[0].view(torch.int32) != 0).float().mean()), 4)}
        same = ops.resolve_voxel_evidence(first)["label"] == ops.resolve_voxel_labels(votes)["label"]
        case["labels_equal_to_hard"] = bool(same.all())
        for k, xs in _time(fns, a.rounds).items():
            case[k] = _stats(xs, N)
        rec["cases"][f"{n}^3"] = case
        del fns, tables, votes, vol, first
        if not a.no_torch:
            del t32, grid
        torch.cuda.empty_cache()
    # ---- the mesh kernel: one view's worth of pixels, V vertices
    V = 200000
    g = torch.Generator(device="cuda").manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"),
                            indexing="ij")
    maps = {"coherent": ((ys // 32) * ((W + 31) // 32) + xs // 32 + 1).to(torch.int32),
            "random": torch.randint(1, V + 1, (H, W), generator=g, device="cuda",
                                    dtype=torch.int32)}
    table = torch.zeros(V, C + 1, dtype=torch.int64, device="cuda")
    fns = {}
    for name, vid in maps.items():
        fns[f"mesh {name}"] = lambda vid=vid: ops.fuse_label_evidence(table, vid, scores[0])
        fns[f"mesh hard {name}"] = lambda vid=vid: ops.fuse_label_votes(table, vid, pred[0])
    for k, xs in _time(fns, a.rounds).items():
        rec["mesh"][k] = _stats(xs, 1)
    print(json.dumps(rec))
    print(f"\nsoft label fusion, ms per {W}x{H} view, C = {C} (median / best of {a.rounds} "
          f"passes); commit {a.commit} (parent {a.parent}), {rec['device']}")
    for name, c in rec["cases"].items():
        print(f"{name:>6} (evidence {c['evidence_MB']} MB, band share {c['band_share']}, labels "
              f"equal to the hard vote's: {c['labels_equal_to_hard']})")
        for k in c:
            if isinstance(c[k], dict):
                print(f"    {k:<20} {c[k]['median_ms_per_view']:.5f} / {c[k]['best']:.5f}")
    print(f"  mesh, {V} vertices")
    for k, c in rec["mesh"].items():
        print(f"    {k:<20} {c['median_ms_per_view']:.5f} / {c['best']:.5f}")


if __name__ == "__main__":
    main()
