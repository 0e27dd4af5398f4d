"""Device time of the depth front end (a record, not a gate).

The frames: 480 x 640, B = 1 / 4 / 16 of them, made from a seed on the device:
a slanted floor, two boxes in front of it (depth steps), Gaussian noise of
0.002 + 0.0005 z^2, millimetre quantisation and 2 % holes.  r = 2 / 3 / 4 with
sigma_space = r / 2.

  fused   one ops.depth.depth_frontend call (filter, points, normals, mask, clean)
  two     ops.depth.filter_depth, then ops.depth.depth_normals of its result, and
          the torch.where that makes clean from the mask
  torch   what it replaces in plain torch: an unfold bilateral filter with exp
          evaluated per tap (no table), then central-difference normals with the
          same depth gate, the camera-facing flip and the same clean

Every call allocates its outputs, as a user's call does.  Alternated in one
process, device events around ``--calls`` calls in a row (one launch of this
size is shorter than an event's resolution is worth), after a warm-up; ms per
call, median / best of ``--rounds``.  It also reports how closely the torch form
agrees: the largest difference of the filtered depth (the table quantises the
range weight into 256 bins over three sigma, the torch form does not) and the
mean angle between the two normals where both forms have one.

    python tools/depth_time.py [--batches 1 4 16] [--radii 2 3 4] [--rounds 5]
        [--calls 20] [--commit ID] [--out profiles/depth_time.txt]
One JSON line, then a table; both are also written to ``--out``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 480, 640
K = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
SIGMA_DEPTH, SIGMA_Z2, MAX_JUMP, MAX_JUMP_Z2, MIN_COS = 0.006, 0.0015, 0.03, 0.004, 0.1
DMIN, DMAX = 1e-6, 3.0e38


def make_frames(B, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32),
                            torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    z = (4.0 - 2.0 * ys / H)[None].repeat(B, 1, 1)                # a slanted floor, 2..4 away
    for b in range(B):
        for (y0, x0, hh, ww, d) in ((120 + 5 * b, 80 + 9 * b, 140, 160, 1.6),
                                    (260 - 3 * b, 380 - 7 * b, 150, 120, 1.2)):
            z[b, y0:y0 + hh, x0:x0 + ww] = d + 0.0004 * xs[y0:y0 + hh, x0:x0 + ww]
    z = z + torch.randn(z.shape, device="cuda", generator=g) * (0.002 + 0.0005 * z * z)
    z = torch.round(z * 1000.0) / 1000.0
    z[torch.rand(z.shape, device="cuda", generator=g) < 0.02] = 0.0
    return z.contiguous()


def time_fns(fns, rounds, calls):
    out = {k: [] for k in fns}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / calls)
    return {k: {"median_ms": round(float(np.median(v)), 4), "best_ms": round(float(np.min(v)), 4)}
            for k, v in out.items()}


def torch_filter(z, r, sigma_space):
    B = z.shape[0]
    ok = torch.isfinite(z) & (z >= DMIN) & (z <= DMAX)
    nan = torch.full_like(z, float("nan"))
    zz = torch.where(ok, z, nan)
    k = torch.arange(-r, r + 1, device=z.device, dtype=torch.float32)
    ws = torch.exp(-(k[:, None] ** 2 + k[None, :] ** 2) / (2.0 * sigma_space ** 2)).reshape(-1)
    pad = torch.nn.functional.pad(zz[:, None], (r, r, r, r), value=float("nan"))
    nb = torch.nn.functional.unfold(pad, 2 * r + 1).view(B, (2 * r + 1) ** 2, H, W)
    d = nb - zz[:, None]
    u = d.abs() / (SIGMA_DEPTH + SIGMA_Z2 * zz * zz)[:, None]
    take = torch.isfinite(d) & (u < 3.0)
    w = torch.where(take, ws[None, :, None, None] * torch.exp(-0.5 * u * u), torch.zeros_like(d))
    d = torch.where(take, d, torch.zeros_like(d))
    return torch.where(ok, zz + (w * d).sum(1) / w.sum(1), torch.zeros_like(z))


def torch_normals(f):
    fx, fy, cx, cy = K
    ok = torch.isfinite(f) & (f >= DMIN) & (f <= DMAX)
    ax = (torch.arange(W, device=f.device, dtype=torch.float32) + 0.5 - cx) / fx
    ay = (torch.arange(H, device=f.device, dtype=torch.float32) + 0.5 - cy) / fy
    P = torch.stack([ax[None, None, :] * f, ay[None, :, None] * f, f], -1)
    thr = MAX_JUMP + MAX_JUMP_Z2 * f * f
    near = lambda a, b, t: (a - b).abs() <= t
    c = f[:, 1:-1, 1:-1]
    t = thr[:, 1:-1, 1:-1]
    good = ok[:, 1:-1, 1:-1] & ok[:, 1:-1, 2:] & ok[:, 1:-1, :-2] & ok[:, 2:, 1:-1] & \
        ok[:, :-2, 1:-1] & near(f[:, 1:-1, 2:], c, t) & near(f[:, 1:-1, :-2], c, t) & \
        near(f[:, 2:, 1:-1], c, t) & near(f[:, :-2, 1:-1], c, t)
    du = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dv = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    n = torch.linalg.cross(dv, du)
    n = n / n.norm(dim=-1, keepdim=True)
    p = P[:, 1:-1, 1:-1]
    dot = (n * p).sum(-1)
    n = torch.where((dot > 0)[..., None], -n, n)
    cosv = dot.abs() / p.norm(dim=-1)
    good = good & torch.isfinite(n).all(-1)
    normals = torch.zeros_like(P)
    normals[:, 1:-1, 1:-1] = torch.where(good[..., None], n, torch.zeros_like(n))
    has = torch.zeros_like(ok)
    has[:, 1:-1, 1:-1] = good
    grazing = torch.zeros_like(ok)
    grazing[:, 1:-1, 1:-1] = good & (cosv < MIN_COS)
    clean = torch.where(ok & has & ~grazing, f, torch.zeros_like(f))
    return P, normals, has, clean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_time.txt"))
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    D = ops.depth
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "calls": a.calls, "frame": [H, W], "cases": {}}
    for B in a.batches:
        z = make_frames(B)
        for r in a.radii:
            tb = D.tables_on(D.bilateral_tables(r, r / 2.0), "cuda")

            def fused():
                return D.depth_frontend(z, tb, K, SIGMA_DEPTH, MAX_JUMP, sigma_z2=SIGMA_Z2,
                                        max_jump_z2=MAX_JUMP_Z2, min_cos=MIN_COS)

            def two():
                f = D.filter_depth(z, tb, SIGMA_DEPTH, SIGMA_Z2)
                n = D.depth_normals(f, K, MAX_JUMP, MAX_JUMP_Z2, MIN_COS)
                n["depth"] = f
                n["clean"] = torch.where((n["mask"] & 12) != 0, torch.zeros_like(f), f)
                return n

            def plain():
                f = torch_filter(z, r, r / 2.0)
                return (f,) + torch_normals(f)

            case = time_fns({"fused": fused, "two": two, "torch": plain}, a.rounds, a.calls)
            x, y, t = fused(), two(), plain()
            same = all(torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)) for k in x)
            both = ((x["mask"] & 2) != 0) & t[3] & ((x["mask"] & 4) == 0)
            cosang = (x["normals"] * t[2]).sum(-1)[both].clamp(-1, 1)
            meas = (x["mask"] & 1) != 0
            case.update(fused_equals_two=bool(same),
                        depth_max_diff=float((x["depth"] - t[0])[meas].abs().max()),
                        depth_mean_diff=float((x["depth"] - t[0])[meas].abs().mean()),
                        normal_mean_angle=float(torch.acos(cosang).mean()),
                        normals_compared=int(both.sum()), pixels=int(z.numel()))
            rec["cases"][f"B{B} r{r}"] = case
            print(f"B {B} r {r}: done", file=sys.stderr, flush=True)
            del x, y, t
            torch.cuda.empty_cache()
    lines = [json.dumps(rec), "",
             f"depth front end, {H} x {W} frames; ms per call, median / best of {a.rounds} windows "
             f"of {a.calls} calls; commit {a.commit}, {rec['device']}",
             "  B  r   fused             two launches      plain torch         fused = two   "
             "torch: depth diff max / mean, normals' mean angle (rad)"]
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, c in rec["cases"].items():
        B, r = name[1:].split(" r")
        lines.append(f"  {B:>2} {r:>2}   {fmt(c, 'fused'):<17} {fmt(c, 'two'):<17} "
                     f"{fmt(c, 'torch'):<19} {str(c['fused_equals_two']):<13} "
                     f"{c['depth_max_diff']:.2e} / {c['depth_mean_diff']:.2e}, "
                     f"{c['normal_mean_angle']:.2e} over {c['normals_compared']} pixels")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
