"""Device time of the voxel-map route (a record, not a gate): 16 views of the
analytic room at H x W against volumes of n^3 over [-3.05, 3.05]^3 (trunc = 4
voxels).  Alternated in one process and timed with device events after a
warm-up; per variant the median and the best ms per view.

  vote hip B     ops.vote_voxel_labels (csrc/voxel_map.hip) with B views per call;
  vote torch     the same rule in plain torch: project, then index_put_ with
                 accumulate into an int32 table (no saturation);
  cast skip      ops.raycast_tsdf, 16 views per call, empty-space skipping (default);
  cast plain     the same with the plain march (same bytes, asserted);
  raster         the mesh route on the same volume: ops.rasterize_mesh of
                 utils.tsdf_fusion.extract_mesh's output (the one-off extraction is
                 reported separately, host clock);
  torch march    a plain-torch marcher: grid_sample of tsdf and of the valid mask
                 at every index of every ray, first crossing by the same secant
                 (not bit-exact; its hit share is reported next to the kernel's).

The ray-cast step is trunc / 2 and the far plane 20.  The whole pass from a
scene directory (scripts/voxel_map_labels.py against fuse_tsdf_mesh.py +
fuse_mesh_labels.py --render) is timed by those scripts' own JSON lines and is
not part of this tool.  One JSON line, then a table.

    python tools/voxel_map_time.py [--sizes 128 256 512] [--B 1 4 16]
        [--H 480 --W 640] [--commit ID] [--parent ID]
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
NEAR, FAR = 0.05, 20.0


def _torch_vote(table, grid, depth, pred, P, intr, trunc):
    """one view, the rule of ucsa_tsdf_vote in plain torch (int32 table [C+1, n])"""
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
    cls = pred.reshape(-1)[pix].long()
    ok &= torch.isfinite(z) & (z >= 1e-6) & (sdf >= -trunc) & (sdf <= trunc) & (cls >= 1) & \
        (cls < table.shape[0])
    vox = torch.nonzero(ok.reshape(-1)).squeeze(1)
    table.index_put_((cls.reshape(-1)[vox], vox),
                     torch.ones(vox.shape[0], dtype=table.dtype, device=table.device),
                     accumulate=True)


def _torch_march(vol, valid, poses, intr, H, W, trunc, step):
    """depth [B,H,W] by grid_sample at every index of every ray"""
    fx, fy, cx, cy = intr
    dev = poses.device
    n = torch.tensor(vol["tsdf"].shape, device=dev, dtype=torch.float32)
    o = torch.tensor(vol["origin"], device=dev)
    h = torch.tensor(vol["spacing"], device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d = torch.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, torch.ones_like(xs)], -1)
    w = torch.einsum("brc,hwc->bhwr", poses[:, :3, :3], d)
    q0 = ((poses[:, :3, 3] - o) / h)[:, None, None, :]
    qd = w / h
    with torch.no_grad():
        z1, z2 = (0 - q0) / qd, ((n - 1) - q0) / qd
        z_in = torch.minimum(z1, z2).amax(-1).clamp_min(NEAR)
        z_out = torch.maximum(z1, z2).amin(-1).clamp_max(FAR)
        dz = step / d.norm(dim=-1)[None]
        steps = int(torch.nan_to_num((z_out - z_in) / dz, 0.0, 0.0, 0.0).clamp_min(0).max()) + 1
        f_vol = vol["tsdf"][None, None]
        m_vol = valid[None, None]
        depth = torch.zeros_like(z_in)
        done = torch.zeros_like(z_in, dtype=torch.bool)

        def sample(z):
            g = q0 + z[..., None] * qd
            # grid_sample: x indexes the last volume axis; align_corners maps -1, 1 to the ends
            p = (2 * g / (n - 1) - 1).flip(-1)[:, None]
            f = torch.nn.functional.grid_sample(f_vol.expand(p.shape[0], -1, -1, -1, -1), p,
                                                align_corners=True)[:, 0, 0]
            m = torch.nn.functional.grid_sample(m_vol.expand(p.shape[0], -1, -1, -1, -1), p,
                                                align_corners=True)[:, 0, 0]
            return f, m >= 1.0
        f0, v0 = sample(z_in)
        for k in range(steps):
            zk, zk1 = z_in + k * dz, z_in + (k + 1) * dz
            f1, v1 = sample(zk1)
            hit = ~done & (zk1 <= z_out) & v0 & v1 & (f0 > 0) & (f1 <= 0)
            depth = torch.where(hit, zk + dz * (f0 / (f0 - f1)), depth)
            done |= hit
            f0, v0 = f1, v1
    return depth


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
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticSceneDataset
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import extract_mesh
    H, W, N = a.H, a.W, a.views
    ds = SyntheticSceneDataset(0, N, H, W)
    intr = [float(v) for v in ds.intrinsics]
    depth = torch.stack([ds[i]["depth"].float() for i in range(N)]).contiguous()
    pred = torch.stack([(ds[i]["label"].long() + 1).clamp(0, 255).to(torch.uint8)
                        for i in range(N)]).contiguous()
    poses = ds.poses.float().contiguous()
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "H": H, "W": W, "views": N, "rounds": a.rounds, "cases": {}}
    for n in a.sizes:
        h = (HI - LO) / (n - 1)
        trunc = 4 * h
        vol = ops.tsdf_volume((n, n, n), (LO,) * 3, h)
        ops.integrate_tsdf(vol, depth, poses, intr, trunc)
        # ---- votes
        tables = {f"vote hip B={b}": ops.voxel_votes(vol, 40) for b in a.B}

        def hip(t, b):
            for s in range(0, N, b):
                ops.vote_voxel_labels(t, vol, depth[s:s + b], pred[s:s + b], poses[s:s + b],
                                      intr, trunc)
        fns = {k: (lambda k=k, b=b: hip(tables[k], b)) for k, b in zip(tables, a.B)}
        if not a.no_torch:
            ax = [LO + torch.arange(n, device="cuda", dtype=torch.float32) * h] * 3
            grid = (ax[0][:, None, None], ax[1][None, :, None], ax[2][None, None, :])
            t32 = torch.zeros(41, n ** 3, dtype=torch.int32, device="cuda")

            def plain():
                for i in range(N):
                    _torch_vote(t32, grid, depth[i], pred[i], poses[i], intr, trunc)
            fns["vote torch"] = plain
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        first = tables[f"vote hip B={a.B[0]}"]
        for k, t in tables.items():
            assert torch.equal(t.view(torch.int16), first.view(torch.int16)), k
        vote_agree = None
        if not a.no_torch:
            vote_agree = int((t32.reshape(first.shape) != first.to(torch.int32)).sum())
        ms = _time(fns, a.rounds)
        case = {"n": n, "votes_MB": round(41 * n ** 3 * 2 / 1e6, 1),
                "torch_votes_differing": vote_agree}
        for k, xs in ms.items():
            xs = np.asarray(xs) / N
            case[k] = {"median_ms_per_view": round(float(np.median(xs)), 5),
                       "best": round(float(xs.min()), 5)}
        del fns, tables
        if not a.no_torch:
            del t32, grid
        labels = ops.resolve_voxel_labels(first)["label"]
        del first
        torch.cuda.empty_cache()
        # ---- model views
        ext = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            verts, faces, _, _ = extract_mesh(vol)
            torch.cuda.synchronize()
            ext.append(1e3 * (time.perf_counter() - t0))
        vlab = torch.ones(verts.shape[0], dtype=torch.int32, device="cuda")
        outs = {}

        def cast(plain):
            outs[plain] = ops.raycast_tsdf(vol, poses, intr, H, W, NEAR, FAR, trunc=trunc,
                                           voxel_labels=labels, _plain_march=plain)
        fns = {"cast skip": lambda: cast(False), "cast plain": lambda: cast(True),
               "raster": lambda: ops.rasterize_mesh(verts, faces, poses, intr, H, W, NEAR,
                                                    vertex_labels=vlab)}
        ms = _time(fns, a.rounds)
        for k in outs[False]:
            assert torch.equal(outs[False][k], outs[True][k]), k
        case["hit_share"] = round(float((outs[False]["voxel_id"] >= 0).float().mean()), 4)
        if not a.no_torch:
            valid = (vol["weight"] >= 1).float()
            tm = _time({"torch march": lambda: outs.__setitem__(
                "torch", _torch_march(vol, valid, poses, intr, H, W, trunc, 0.5 * trunc))}, 2)
            ms.update(tm)
            case["torch_march_hit_share"] = round(float((outs["torch"] > 0).float().mean()), 4)
        for k, xs in ms.items():
            xs = np.asarray(xs) / N
            case[k] = {"median_ms_per_view": round(float(np.median(xs)), 5),
                       "best": round(float(xs.min()), 5)}
        case["extract_ms"] = {"median": round(float(np.median(ext)), 3),
                              "best": round(float(np.min(ext)), 3)}
        case["faces"] = int(faces.shape[0])
        rec["cases"][f"{n}^3"] = case
        del vol, labels, outs, verts, faces, fns
        torch.cuda.empty_cache()
    print(json.dumps(rec))
    print(f"\nvoxel map, ms per {W}x{H} view (median / best of {a.rounds} passes over {N} views; "
          f"torch march: 2 passes); extraction ms per volume; commit {a.commit} (parent "
          f"{a.parent}), {rec['device']}")
    for name, c in rec["cases"].items():
        keys = [k for k in c if isinstance(c[k], dict) and "median_ms_per_view" in c[k]]
        print(f"{name:>6} (votes {c['votes_MB']} MB, {c['faces']} faces, hit share "
              f"{c['hit_share']})")
        for k in keys:
            print(f"    {k:<16} {c[k]['median_ms_per_view']:.5f} / {c[k]['best']:.5f}")
        print(f"    {'extract (once)':<16} {c['extract_ms']['median']:.3f} / "
              f"{c['extract_ms']['best']:.3f}")
    print("    whole pass from a scene directory to map_label/: not measured")


if __name__ == "__main__":
    main()
