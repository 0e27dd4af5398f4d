"""Device time of the occupancy prior and what it buys the marcher (a record,
not a gate).

1. The op: 16 views of the analytic room (H x W) fused into volumes of n^3 over
   [-3.05, 3.05]^3 (trunc = 4 voxels), then the mask for bound 4, 128^3 cells,
   3 cascades, default dilate, unknown = "keep":

     hip    ops.tsdf_occupancy (csrc/occupancy_prior.hip): pack + one lane per cell;
     torch  what one would write without the kernel: the blocking mask dilated by
            one voxel (max_pool3d, kernel 3), padded / cropped to each cascade's
            box in voxel indices and resampled to 128^3 by adaptive_max_pool3d.
            It is not the contract (its cell borders are rounded to voxels); the
            share of cells on which it agrees with the kernel is reported.

   Alternated in one process, device events, after a warm-up; median / best.
2. Training through the marcher (the loop of
   test_field_trained_through_the_marcher_quality_and_sparsity: 4096 rays,
   refresh_due refreshes included) with and without the prior made from the
   dataset's own depth frames (unknown = "empty", default dilate): mean ms per
   step over the first 600 steps, steady-state ms per step over steps 600..800,
   points per step over the first 128 steps.  Runs alternate; host clock around
   windows that end in a device synchronise.

    python tools/occupancy_prior_time.py [--sizes 128 256 512] [--rounds 9]
        [--train_rounds 3] [--commit ID]
One JSON line, then a table."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI, BOUND, GRID = -3.05, 3.05, 4.0, 128


def torch_occupancy(vol, h, cascade=3):
    blocked = ~((vol["weight"] >= 1.0) & (vol["tsdf"] >= 1.0))
    x = F.max_pool3d(blocked[None, None].float(), 3, 1, 1)
    out = []
    for cas in range(cascade):
        b = min(2.0 ** cas, BOUND)
        i0, i1 = int(np.floor((-b - LO) / h + 0.5)), int(np.ceil((b - LO) / h + 0.5))
        n = x.shape[-1]
        lo_pad, hi_pad = max(0, -i0), max(0, i1 - n)
        y = F.pad(x, (lo_pad, hi_pad) * 3, value=1.0) if lo_pad or hi_pad else x
        a, e = i0 + lo_pad, i1 + lo_pad
        out.append(F.adaptive_max_pool3d(y[..., a:e, a:e, a:e], GRID)[0, 0] > 0)
    return torch.stack(out).to(torch.uint8)


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
    return out


def train_run(ds, mask, steps=800, early=600, rays=4096):
    import bench
    from ucsa_neural_rendering_amd import losses as ul
    from ucsa_neural_rendering_amd.nerf.network_tcnn_semantics import SemanticNeRFNetwork
    from ucsa_neural_rendering_amd.nerf.optim import HipAdam
    dev = torch.device("cuda:0")
    net = SemanticNeRFNetwork(encoding="hashgrid", bound=4, cuda_ray=True,
                              num_semantic_classes=bench.N_CLASSES, seed=123).to(dev).train()
    net.march_training = True
    if mask is not None:
        net.set_occupancy_prior(mask)
    opt = HipAdam(
        [{"name": "encoding", "params": list(net.encoder.parameters())},
         {"name": "net", "params": list(net.sigma_net.parameters()) +
          list(net.color_net.parameters()) + list(net.semantics_net.parameters()),
          "weight_decay": 1e-6}], lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    g = torch.Generator(device=dev).manual_seed(1)
    points = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(steps):
        if it == early:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        if net.refresh_due(it):
            if 0 < it <= 128:
                points.append(net.step_counter[:net.local_step, 0].clone())
            net.update_extra_state()
        item = ds[it % len(ds)]
        inds = torch.randint(0, ds.H * ds.W, (rays,), device=dev, generator=g)
        out = net.render(item["rays_o"][inds][None], item["rays_d"][inds][None],
                         item["direction_norms"][inds][None], perturb=True, dt_gamma=1 / 256)
        lc, ls, ld = ul.nerf_losses(
            out["image"], out["semantics"], out["depth"],
            item["img"].reshape(3, -1).t()[inds][None], item["label"].reshape(-1)[inds][None],
            item["depth"].float().reshape(-1)[inds][None], 1.0)
        loss = ul.nerf_total_loss(lc, ls, ld)
        opt.zero_grad()
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return {"early_ms_per_step": 1e3 * (t1 - t0) / early,
            "steady_ms_per_step": 1e3 * (t2 - t1) / (steps - early),
            "points_per_step_first_128": float(torch.cat(points).double().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--train_rounds", type=int, default=3)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticSceneDataset
    from ucsa_neural_rendering_amd.utils.occupancy_prior import prior_from_depth_views
    import bench
    ds = SyntheticSceneDataset(0, n_views=16, H=a.H, W=a.W, n_classes=bench.N_CLASSES)
    intr = [float(v) for v in ds.intrinsics]
    depth = torch.stack([ds[i]["depth"].float() for i in range(16)]).contiguous()
    poses = ds.poses.float().contiguous()
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "H": a.H, "W": a.W,
           "rounds": a.rounds, "op": {}, "train": {}}
    for n in a.sizes:
        h = (HI - LO) / (n - 1)
        vol = ops.tsdf_volume((n, n, n), (LO,) * 3, h)
        ops.integrate_tsdf(vol, depth, poses, intr, 4 * h)
        fns = {"hip": lambda: ops.tsdf_occupancy(vol, BOUND),
               "torch": lambda: torch_occupancy(vol, h)}
        got, plain = fns["hip"](), fns["torch"]()
        ms = time_fns(fns, a.rounds)
        case = {"kept": [round(float(v), 4) for v in got.float().mean((1, 2, 3)).tolist()],
                "torch_agrees_on": round(float((got == plain).float().mean()), 4)}
        for k, xs in ms.items():
            case[k] = {"median_ms": round(float(np.median(xs)), 4),
                       "best_ms": round(float(np.min(xs)), 4)}
        rec["op"][f"{n}^3"] = case
        del vol, fns, got, plain
        torch.cuda.empty_cache()
    dmaps = [d.cpu().numpy() for d in depth]
    mask, st = prior_from_depth_views(poses.cpu().numpy(), intr, a.H, a.W, dmaps, BOUND,
                                      unknown="empty")
    rec["train"]["kept"] = [round(v, 4) for v in st["kept"]]
    rec["train"]["prior_ms"] = {"integrate": round(st["integrate_ms"], 3),
                                "occupancy": round(st["occupancy_ms"], 3)}
    train_run(ds, None, steps=64, early=32)  # warm-up: code objects, workspaces
    runs = {"plain": [], "prior": []}
    for _ in range(a.train_rounds):
        runs["plain"].append(train_run(ds, None))
        runs["prior"].append(train_run(ds, mask))
    for k, rs in runs.items():
        rec["train"][k] = {q: {"median": round(float(np.median([r[q] for r in rs])), 4),
                               "best": round(float(np.min([r[q] for r in rs])), 4)}
                           for q in rs[0]}
    print(json.dumps(rec))
    print(f"\nucsa_tsdf_occupancy, room volumes, bound 4, 3 x 128^3 cells; ms median / best of "
          f"{a.rounds}; commit {a.commit}, {rec['device']}")
    for name, c in rec["op"].items():
        print(f"{name:>6}  hip {c['hip']['median_ms']:.4f} / {c['hip']['best_ms']:.4f}   torch "
              f"{c['torch']['median_ms']:.4f} / {c['torch']['best_ms']:.4f}   kept {c['kept']}   "
              f"torch agrees on {c['torch_agrees_on']}")
    print(f"\ntraining through the marcher, 800 steps of 4096 rays, median / best of "
          f"{a.train_rounds} runs; prior kept {rec['train']['kept']}, made in "
          f"{rec['train']['prior_ms']} ms")
    for k in ("plain", "prior"):
        t = rec["train"][k]
        print(f"{k:>6}  first 600 steps {t['early_ms_per_step']['median']:.3f} / "
              f"{t['early_ms_per_step']['best']:.3f} ms per step   steady "
              f"{t['steady_ms_per_step']['median']:.3f} / {t['steady_ms_per_step']['best']:.3f}   "
              f"points per step over the first 128 steps "
              f"{t['points_per_step_first_128']['median']:.0f}")


if __name__ == "__main__":
    main()
