"""Device time of the mesh voxelization and what a mesh prior buys the marcher (a
record, not a gate).

1. The op on the analytic room's meshes (SyntheticRoom(0).labelled_mesh at steps
   1.0 / 0.25 / 0.05 / 0.02): ``ops.mesh_occupancy`` (bound 4, 3 x 128^3 cells,
   default dilate) and ``ops.voxelize_mesh`` on n^3 lattices over
   [-3.05, 3.05]^3, whole op (count, torch's prefix sum with its read-back, fill)
   and the two kernels on their own through the C entries.  Against

     torch  what one would write without the kernel: ``ops.sample_mesh_surface``
            dense enough for about four points per finest-cell face area, each
            point's cell by floor, a scatter of ones.  It is not conservative (a
            cell a face only clips gets no sample, and no dilate), so the share
            of cells on which it agrees with the kernel is reported, not held
            to 100 %;
     depth  the depth route's integrate_ms + occupancy_ms for the same scene
            (``prior_from_depth_views``, the protocol of occupancy_prior_time.py).

   Alternated in one process, device events, after a warm-up; median / best.
2. Training through the marcher (occupancy_prior_time.py's loop: 4096 rays, 800
   steps, refreshes included) three ways: no prior, the TSDF prior with
   unknown = "empty", and the mesh prior from the TSDF-fused mesh of the same
   frames: ms per step over the first 600 steps and over steps 600..800, points
   per step over the first 128 steps, PSNR / mIoU of 8 marched views after 800.

    python tools/voxelize_time.py [--steps 1.0 0.25 0.05 0.02] [--sizes 128 256 512]
        [--rounds 9] [--train_rounds 2] [--commit ID]
One JSON line, then a table."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI, BOUND, GRID, CASCADE = -3.05, 3.05, 4.0, 128, 3


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


def kernels(v, f, family, dims, origin, spacing, bound, cascade, dilate):
    """the count and the fill entry as two closures on prepared buffers"""
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    nf, items = int(f.shape[0]), int(f.shape[0]) * cascade
    ws = torch.empty(3 * items, dtype=torch.int64, device="cuda")
    count = torch.empty(items, dtype=torch.int32, device="cuda")
    cells = cascade * dims[0] * dims[1] * dims[2]
    mask = torch.empty(cells, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    geo = (p(v), int(v.shape[0]), p(f), nf, family, *dims,
           _lib.fvec(origin) if origin else None, _lib.fvec(spacing) if spacing else None,
           bound, cascade, dilate)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run_count():
        _lib.check(l.ucsa_mesh_voxelize_count(*geo, p(count), p(ws), 24 * items, stream), "count")

    run_count()
    first = torch.zeros(items + 1, dtype=torch.int64, device="cuda")
    first[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    total = int(first[items])

    def run_fill():
        _lib.check(l.ucsa_mesh_voxelize_fill(*geo, p(first), total, 0, p(mask), cells, p(ws),
                                             24 * items, stream), "fill")

    return run_count, run_fill, total


def torch_occupancy(ops, v, f, density):
    pts = ops.sample_mesh_surface(v, f, density, seed=0)["points"]
    out = torch.zeros(CASCADE, GRID, GRID, GRID, dtype=torch.uint8, device=v.device)
    for cas in range(CASCADE):
        b = min(2.0 ** cas, BOUND)
        idx = torch.floor((pts / b + 1.0) * (0.5 * GRID)).long()
        ok = ((idx >= 0) & (idx < GRID)).all(1)
        i = idx[ok]
        out[cas].view(-1)[(i[:, 0] * GRID + i[:, 1]) * GRID + i[:, 2]] = 1
    return out


def train_run(ds, mask, steps=800, early=600, rays=4096, score=True):
    import bench
    from ucsa_neural_rendering_amd import losses as ul
    from ucsa_neural_rendering_amd.nerf.network_tcnn_semantics import SemanticNeRFNetwork
    from ucsa_neural_rendering_amd.nerf.optim import HipAdam
    from ucsa_neural_rendering_amd.utils.metrics import SemanticsMeter
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
    res = {"early_ms_per_step": 1e3 * (t1 - t0) / early,
           "steady_ms_per_step": 1e3 * (t2 - t1) / (steps - early),
           "points_per_step_first_128": float(torch.cat(points).double().mean())}
    if score:
        net.eval()
        net.update_extra_state()
        meter, ps = SemanticsMeter(bench.N_CLASSES), []
        for v in (0, 2, 4, 6, 8, 10, 12, 14):
            it = ds[v]
            with torch.no_grad():
                o = net.render(it["rays_o"][None], it["rays_d"][None], it["direction_norms"][None],
                               dt_gamma=1 / 256, far_closure=False)
            gt = it["img"].reshape(3, -1).t()
            ps.append(float(-10 * torch.log10(((o["image"][0] - gt) ** 2).mean())))
            meter.update(o["semantics"][0].argmax(-1).cpu(), it["label"].reshape(-1).cpu())
        res.update(psnr=sum(ps) / len(ps), miou=float(meter.measure()[0]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[1.0, 0.25, 0.05, 0.02])
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=320)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--train_rounds", type=int, default=2)
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import bench
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import (SyntheticRoom,
                                                                   SyntheticSceneDataset)
    from ucsa_neural_rendering_amd.utils.occupancy_prior import (prior_from_depth_views,
                                                                 prior_from_mesh)
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import fuse_depth_views
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "op": {}, "train": {}}
    room = SyntheticRoom(0)
    dilate = 2.0 / GRID
    # about four points per finest-cell face: the finest cell is 2 / 128 wide
    density = 4.0 / (2.0 / GRID) ** 2
    for step in a.steps:
        m = room.labelled_mesh(step)
        v = torch.from_numpy(m["verts"].astype(np.float32)).cuda()
        f = torch.from_numpy(m["faces"].astype(np.int32)).cuda()
        case = {"faces": int(f.shape[0])}
        cnt, fill, total = kernels(v, f, 1, (GRID,) * 3, None, None, BOUND, CASCADE, dilate)
        fns = {"whole": lambda: ops.mesh_occupancy(v, f, BOUND), "count": cnt, "fill": fill,
               "torch": lambda: torch_occupancy(ops, v, f, density)}
        got, plain = fns["whole"](), fns["torch"]()
        case["mesh_occupancy"] = {"columns": total, **time_fns(fns, a.rounds),
                                  "kept": [round(float(x), 4)
                                           for x in got.float().mean((1, 2, 3)).tolist()],
                                  "torch_agrees_on": round(float((got == plain).float().mean()), 4),
                                  "torch_cells_not_in_kernel": int(((plain != 0) & (got == 0)).sum())}
        for n in a.sizes:
            h = (HI - LO) / (n - 1)
            cnt, fill, total = kernels(v, f, 0, (n,) * 3, (LO,) * 3, (h,) * 3, 0.0, 1, 0.0)
            fns = {"whole": lambda: ops.voxelize_mesh(v, f, (n,) * 3, (LO,) * 3, h),
                   "count": cnt, "fill": fill}
            got = fns["whole"]()
            case[f"voxelize_{n}^3"] = {"columns": total, **time_fns(fns, a.rounds),
                                       "kept": round(float(got.float().mean()), 5)}
            del got, fns, cnt, fill
            torch.cuda.empty_cache()
        rec["op"][f"step {step}"] = case
        print(f"step {step}: done", file=sys.stderr, flush=True)
    ds = SyntheticSceneDataset(0, n_views=16, H=a.H, W=a.W, n_classes=bench.N_CLASSES)
    intr = [float(x) for x in ds.intrinsics]
    dmaps = [ds[i]["depth"].float().cpu().numpy() for i in range(16)]
    poses = ds.poses.float().cpu().numpy()
    mesh = fuse_depth_views(poses, intr, a.H, a.W, dmaps)
    for _ in range(2):   # the second call of each: warm
        tsdf_mask, st = prior_from_depth_views(poses, intr, a.H, a.W, dmaps, BOUND,
                                               unknown="empty")
        mesh_mask, ms = prior_from_mesh(mesh["verts"], mesh["faces"], BOUND)
    rec["train"]["priors"] = {
        "tsdf": {"kept": [round(x, 4) for x in st["kept"]],
                 "integrate_ms": round(st["integrate_ms"], 3),
                 "occupancy_ms": round(st["occupancy_ms"], 3)},
        "mesh": {"kept": [round(x, 4) for x in ms["kept"]], "faces": ms["faces"],
                 "voxelize_ms": round(ms["voxelize_ms"], 3)},
        "mesh_cells_outside_tsdf": round(float(((mesh_mask != 0) & (tsdf_mask == 0))
                                               .float().mean()), 4),
        "tsdf_cells_outside_mesh": round(float(((tsdf_mask != 0) & (mesh_mask == 0))
                                               .float().mean()), 4)}
    train_run(ds, None, steps=64, early=32, score=False)  # warm-up: code objects, workspaces
    ways = {"plain": None, "tsdf": tsdf_mask, "mesh": mesh_mask}
    runs = {k: [] for k in ways}
    for _ in range(a.train_rounds):
        for k, mask in ways.items():
            runs[k].append(train_run(ds, mask))
            print(f"train {k}: done", file=sys.stderr, flush=True)
    for k, rs in runs.items():
        rec["train"][k] = {q: {"median": round(float(np.median([r[q] for r in rs])), 4),
                               "best": round(float(np.min([r[q] for r in rs])), 4)}
                           for q in rs[0]}
    print(json.dumps(rec))
    print(f"\nmesh voxelization, room meshes; ms median / best of {a.rounds}; commit {a.commit}, "
          f"{rec['device']}")
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, case in rec["op"].items():
        c = case["mesh_occupancy"]
        print(f"{name} ({case['faces']} faces)\n  mesh_occupancy 3 x 128^3: whole {fmt(c, 'whole')}   "
              f"count {fmt(c, 'count')}   fill {fmt(c, 'fill')} ({c['columns']} columns)   torch "
              f"{fmt(c, 'torch')}, agrees on {c['torch_agrees_on']}, "
              f"{c['torch_cells_not_in_kernel']} of its cells not in the kernel's   kept {c['kept']}")
        for n in a.sizes:
            c = case[f"voxelize_{n}^3"]
            print(f"  voxelize_mesh {n}^3: whole {fmt(c, 'whole')}   count {fmt(c, 'count')}   fill "
                  f"{fmt(c, 'fill')} ({c['columns']} columns)   kept {c['kept']}")
    p = rec["train"]["priors"]
    print(f"\npriors for bound 4: tsdf (unknown = empty) kept {p['tsdf']['kept']}, integrate "
          f"{p['tsdf']['integrate_ms']} + occupancy {p['tsdf']['occupancy_ms']} ms; mesh "
          f"({p['mesh']['faces']} faces of the TSDF-fused mesh) kept {p['mesh']['kept']}, voxelize "
          f"{p['mesh']['voxelize_ms']} ms; share of cells in mesh only {p['mesh_cells_outside_tsdf']}, "
          f"in tsdf only {p['tsdf_cells_outside_mesh']}")
    print(f"training through the marcher, 800 steps of 4096 rays, median / best of "
          f"{a.train_rounds} runs")
    for k in ways:
        t = rec["train"][k]
        print(f"{k:>6}  first 600 steps {t['early_ms_per_step']['median']:.3f} / "
              f"{t['early_ms_per_step']['best']:.3f} ms per step   steady "
              f"{t['steady_ms_per_step']['median']:.3f} / {t['steady_ms_per_step']['best']:.3f}   "
              f"points per step over the first 128 steps "
              f"{t['points_per_step_first_128']['median']:.0f}   PSNR {t['psnr']['median']:.2f}   "
              f"mIoU {t['miou']['median']:.4f}")


if __name__ == "__main__":
    main()
