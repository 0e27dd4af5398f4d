"""Device time of the TSDF integration and of the mesh extraction (a record, not
a gate): 16 views of the analytic room at H x W fused into volumes of n^3 over
[-3.05, 3.05]^3 (trunc = 4 voxels), with and without colour.  Alternated in one
process and timed with device events after a warm-up:

  hip B    ops.integrate_tsdf (csrc/tsdf_fusion.hip) with B views per call: the
           voxel state is read and written once per call;
  torch    what one would write without the kernel: the same update per view as
           a dozen element-wise launches and a gather over the whole volume
           (fp32, same order of operations; its volume is compared with the
           kernel's before timing and
           the difference is reported).

Each round times one pass over all views with one variant; ``--rounds`` rounds
per variant, interleaved.  Per variant: the median and the best ms per view.
Then the extraction (mask weight >= 1 + masked ops.marching_cubes; host clock,
synchronised: it reads the totals back between its passes).  One JSON line,
then a table.

    python tools/tsdf_time.py [--sizes 128 256 512] [--B 1 4 16] [--H 480 --W 640]
        [--commit ID]
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

LO, HI = -3.05, 3.05


def _torch_view(vol, grid, depth, color, P, intr, trunc, max_weight):
    """one view, the contract of ucsa_tsdf_integrate in plain torch"""
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
    ok &= torch.isfinite(z) & (z >= 1e-6) & ~(sdf < -trunc)
    x = torch.clamp_max(sdf / trunc, 1.0)
    w = vol["weight"]
    w1 = w + 1.0
    vol["tsdf"].copy_(torch.where(ok, (vol["tsdf"] * w + x) / w1, vol["tsdf"]))
    if color is not None:
        col = color.reshape(-1, 3)[pix].float()
        vol["rgb"].copy_(torch.where(ok[..., None], (vol["rgb"] * w[..., None] + col) /
                                     w1[..., None], vol["rgb"]))
    w.copy_(torch.where(ok, torch.clamp_max(w1, max_weight), w))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--no_torch", action="store_true")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticSceneDataset
    H, W, N = a.H, a.W, a.views
    ds = SyntheticSceneDataset(0, N, H, W)
    intr = [float(v) for v in ds.intrinsics]
    depth = torch.stack([ds[i]["depth"].float() for i in range(N)]).contiguous()
    color = torch.stack([(ds[i]["img"].permute(1, 2, 0) * 255.0).round().to(torch.uint8)
                         for i in range(N)]).contiguous()
    poses = ds.poses.float().contiguous()
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "H": H, "W": W,
           "views": N, "rounds": a.rounds, "cases": {}}
    for n in a.sizes:
        h = (HI - LO) / (n - 1)
        trunc = 4 * h
        for with_color in (False, True):
            col = color if with_color else None
            vols = {k: ops.tsdf_volume((n, n, n), (LO,) * 3, h, with_color)
                    for k in [f"hip B={b}" for b in a.B] + ([] if a.no_torch else ["torch"])}

            def hip(vol, b):
                for s in range(0, N, b):
                    ops.integrate_tsdf(vol, depth[s:s + b], poses[s:s + b], intr, trunc,
                                       color=None if col is None else col[s:s + b])

            fns = {f"hip B={b}": (lambda b=b: hip(vols[f"hip B={b}"], b)) for b in a.B}
            if not a.no_torch:
                ax = [LO + torch.arange(n, device="cuda", dtype=torch.float32) * h] * 3
                grid = (ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :])

                def plain():
                    for i in range(N):
                        _torch_view(vols["torch"], grid, depth[i],
                                    None if col is None else col[i], poses[i], intr, trunc,
                                    65504.0)
                fns["torch"] = plain
            for fn in fns.values():
                fn()
            torch.cuda.synchronize()
            first = vols[f"hip B={a.B[0]}"]
            agree = None
            for k, vol in vols.items():
                same = all(torch.equal(vol[q], first[q]) for q in ("tsdf", "weight"))
                if k.startswith("hip"):
                    assert same, k
                else:
                    # reported, not asserted: torch's own division need not round as
                    # the contract asks
                    agree = {"max_abs_tsdf": float((vol["tsdf"] - first["tsdf"]).abs().max()),
                             "weights_differing": int((vol["weight"] != first["weight"]).sum())}
            # the extraction, on the volume after one pass
            ext = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                valid = first["weight"] >= 1
                verts, faces, _ = ops.marching_cubes(-first["tsdf"], 0.0, first["origin"],
                                                     first["spacing"], valid=valid)
                torch.cuda.synchronize()
                ext.append(1e3 * (time.perf_counter() - t0))
            ms = _time(fns, a.rounds)
            case = {"n": n, "color": with_color, "state_MB": round(n ** 3 * (20 if with_color
                                                                             else 8) / 1e6, 1),
                    "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]),
                    "torch_vs_hip": agree,
                    "extract_ms": {"median": round(float(np.median(ext)), 3),
                                   "best": round(float(np.min(ext)), 3)}}
            for k, xs in ms.items():
                xs = np.asarray(xs) / N
                case[k] = {"median_ms_per_view": round(float(np.median(xs)), 5),
                           "best": round(float(xs.min()), 5)}
            rec["cases"][f"{n}^3 {'rgb' if with_color else 'plain'}"] = case
            del vols, first, fns
            torch.cuda.empty_cache()
    print(json.dumps(rec))
    print(f"\nintegration, ms per {W}x{H} view (median / best of {a.rounds} passes over {N} "
          f"views); extraction ms per volume; commit {a.commit}, {rec['device']}")
    for name, c in rec["cases"].items():
        cols = "  ".join(f"{k} {c[k]['median_ms_per_view']:.5f} / {c[k]['best']:.5f}"
                         for k in c if k.startswith("hip") or k == "torch")
        print(f"{name:>12} ({c['state_MB']:>7} MB)  {cols}  extract "
              f"{c['extract_ms']['median']:.3f} / {c['extract_ms']['best']:.3f} "
              f"(V={c['vertices']})")


if __name__ == "__main__":
    main()
