"""Device time of the ICP step against a TSDF volume (a record, not a gate).

The volume: eight 480 x 640 views of a loop through SyntheticRoom(0), z-depth
from the room's own ray cast, integrated at their true poses into a lattice of
n^3 over [-3.05, 3.05]^3 with trunc = 4 voxels, n = 128 and 256.  The frame: a
ninth view of the loop, back-projected at strides 1 (307 200 pixels) and 4, in
pixel order and shuffled, under a pose 1 degree and 0.02 away from its own.

  fused     one ops.register.tsdf_sums call: transform, sixteen loads, 29 sums
  torch     what it replaces in plain torch: the transform, the sixteen explicit
            gathers, the same value, gradient, r and J, float64 sums of the same
            29 terms (no fixed tree)
  mesh      the mesh route: ops.register.icp_sums against extract_mesh of the same
            volume at max_dist = trunc; its one-off work (extract_mesh,
            triangle_grid, face_unit_normals) is listed separately
  refine    a whole utils.registration.refine_pose_tsdf call from that pose
            (back-projection and every 29-double read included)
  integrate one ops.integrate_tsdf call of the frame: what a frame costs without
            tracking; refine + integrate is what it costs with it

Alternated in one process, device events, after a warm-up; median / best.

    python tools/tsdf_register_time.py [--dims 128 256] [--rounds 5] [--commit ID]
        [--out profiles/tsdf_register_time.txt]
One JSON line, then a table; both are also written to ``--out``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.register_time import PAIRS, move, time_fns  # noqa: E402

H, W, VIEWS, FRAME = 480, 640, 8, 8


def cast_depth(room, pose, K):
    """z-depth [H,W] of the analytic room through the pixel centres, on the room's device"""
    fx, fy, cx, cy = K
    dev = room.room.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d = torch.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, torch.ones_like(xs)], -1)
    d = d.reshape(-1, 3)
    nrm = d.norm(dim=1)
    P = torch.as_tensor(pose, dtype=torch.float32, device=dev)
    dw = (d / nrm[:, None]) @ P[:3, :3].T
    t = room.cast(P[:3, 3].expand_as(dw).contiguous(), dw.contiguous())[0]
    return (t / nrm).reshape(H, W)


def torch_sums(vol, pts, T32, trunc, min_weight, max_tsdf):
    """the step in plain torch: the same expressions, float64 sums (no fixed tree)"""
    tsdf, weight = vol["tsdf"].reshape(-1), vol["weight"].reshape(-1)
    nx, ny, nz = vol["tsdf"].shape
    o = torch.tensor(vol["origin"], device=pts.device)
    h = torch.tensor(vol["spacing"], device=pts.device)
    q = move(pts, T32)
    g = (q - o) / h
    top = torch.tensor([nx - 1.0, ny - 1.0, nz - 1.0], device=pts.device)
    inside = ((g >= 0) & (g <= top)).all(1)
    fl = torch.minimum(torch.floor(torch.where(inside[:, None], g, torch.zeros_like(g))), top - 1)
    f = torch.where(inside[:, None], g, torch.zeros_like(g)) - fl
    c = fl.long()
    base = (c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]
    offs = [i * ny * nz + j * nz + k for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    w = [weight[base + d] for d in offs]                       # eight gathers
    v = [tsdf[base + d] for d in offs]                         # and eight more
    observed = inside
    for x in w:
        observed = observed & (x >= min_weight)
    lerp = lambda x, y, s: x + s * (y - x)
    c00, c01 = lerp(v[0], v[1], f[:, 2]), lerp(v[2], v[3], f[:, 2])
    c10, c11 = lerp(v[4], v[5], f[:, 2]), lerp(v[6], v[7], f[:, 2])
    c0, c1 = lerp(c00, c01, f[:, 1]), lerp(c10, c11, f[:, 1])
    Fv = lerp(c0, c1, f[:, 0])
    G = torch.stack([c1 - c0, lerp(c01 - c00, c11 - c10, f[:, 0]),
                     lerp(lerp(v[1] - v[0], v[3] - v[2], f[:, 1]),
                          lerp(v[5] - v[4], v[7] - v[6], f[:, 1]), f[:, 0])], 1) / h
    ln = G.norm(dim=1)
    hit = observed & (ln > 0) & torch.isfinite(ln) & (Fv.abs() <= max_tsdf)
    n = torch.where(hit[:, None], G / ln[:, None], torch.zeros_like(G))
    r = torch.where(hit, -(Fv * trunc), torch.zeros_like(Fv)).double()
    J = torch.where(hit[:, None], torch.cat([torch.linalg.cross(q, n), n], 1),
                    torch.zeros(1, device=pts.device)).double()
    cols = [(J[:, a] * J[:, b]).sum() for a, b in PAIRS] + \
        [(J[:, a] * r).sum() for a in range(6)] + [(r * r).sum(), hit.double().sum()]
    return torch.stack(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_register_time.txt"))
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, _slerp_loop_poses
    from ucsa_neural_rendering_amd.utils import registration as REG
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import extract_mesh
    room = SyntheticRoom(0).to("cuda")
    poses = _slerp_loop_poses(VIEWS + 1, seed=123).numpy().astype(np.float32)
    K = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    depth = torch.stack([cast_depth(room, poses[b], K) for b in range(VIEWS + 1)]).contiguous()
    pose = poses[FRAME].astype(np.float64)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    T = REG.compose(pose, np.concatenate([np.radians(1.0) * axis, [0.012, -0.012, 0.0106]]))
    T32 = torch.from_numpy(T[:3].astype(np.float32)).cuda()
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "frame": [H, W], "views": VIEWS, "cases": {}}
    gen = torch.Generator(device="cuda").manual_seed(0)
    for n in a.dims:
        h = 6.1 / (n - 1)
        trunc = 4.0 * h
        vol = ops.tsdf_volume((n, n, n), [-3.05] * 3, h, device="cuda")
        ops.integrate_tsdf(vol, depth[:VIEWS], torch.from_numpy(poses[:VIEWS]).cuda(), K, trunc)
        one = {}
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k in range(2):                                      # the second pass is the record
            t0.record()
            mv, mf, _, _ = extract_mesh(vol, 1)
            t1.record()
            t1.synchronize()
            one["extract_mesh_ms"] = round(t0.elapsed_time(t1), 4)
            t0.record()
            grid = ops.triangle_grid(mv, mf)
            unit = ops.register.face_unit_normals(mv, mf)
            t1.record()
            t1.synchronize()
            one["triangle_grid_ms"] = round(t0.elapsed_time(t1), 4)
        case = {"voxel": round(h, 5), "trunc": round(trunc, 5), "faces": int(mf.shape[0]),
                "one_off": one}
        frame = depth[FRAME]
        Pf = torch.from_numpy(poses[FRAME:FRAME + 1]).cuda()
        for stride in (1, 4):
            pix = REG.backproject(frame, K, stride)
            shuf = pix[torch.randperm(pix.shape[0], device="cuda", generator=gen)].contiguous()
            tsdf_sums, icp = ops.register.tsdf_sums, ops.register.icp_sums
            fns = {"fused": lambda: tsdf_sums(vol, pix, T, trunc),
                   "fused shuffled": lambda: tsdf_sums(vol, shuf, T, trunc),
                   "torch": lambda: torch_sums(vol, pix, T32, trunc, 1.0, 1.0),
                   "torch shuffled": lambda: torch_sums(vol, shuf, T32, trunc, 1.0, 1.0),
                   "mesh": lambda: icp(grid, mv, mf, unit, pix, T, trunc),
                   "mesh shuffled": lambda: icp(grid, mv, mf, unit, shuf, T, trunc),
                   "refine": lambda: REG.refine_pose_tsdf(frame, T, K, vol, trunc, stride=stride)}
            if stride == 1:
                scratch = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vol.items()}
                fns["integrate"] = lambda: ops.integrate_tsdf(scratch, frame[None], Pf, K, trunc)
            sub = time_fns(fns, a.rounds)
            out = REG.refine_pose_tsdf(frame, T, K, vol, trunc, stride=stride)
            rot, trans = REG.pose_step(out["pose"], pose)
            s_f = tsdf_sums(vol, pix, T, trunc).cpu().numpy()
            s_t = torch_sums(vol, pix, T32, trunc, 1.0, 1.0).cpu().numpy()
            sub.update(points=int(pix.shape[0]), matched=out["matched"], rank=out["rank"],
                       iterations=out["iterations"], converged=out["converged"],
                       rmse=out["rmse"], first_rmse=out["history"][0]["rmse"],
                       error_rad=rot, error_units=trans,
                       torch_rel_diff=float(np.abs(s_f - s_t).max() / np.abs(s_f).max()))
            case[f"stride {stride}"] = sub
            del fns
        rec["cases"][f"{n}^3"] = case
        print(f"{n}^3: done", file=sys.stderr, flush=True)
        del vol, grid
        torch.cuda.empty_cache()
    lines = [json.dumps(rec), "",
             f"ICP step against a TSDF volume, one {H} x {W} frame 1 deg / 0.02 off, volume of "
             f"{VIEWS} such views; ms median / best of {a.rounds}; commit {a.commit}, "
             f"{rec['device']}"]
    fmt = lambda c, k: f"{c[k]['median_ms']:.4f} / {c[k]['best_ms']:.4f}"
    for name, c in rec["cases"].items():
        lines.append(f"{name} (voxel {c['voxel']}, trunc {c['trunc']}); the mesh route's one-off "
                     f"work: extract_mesh {c['one_off']['extract_mesh_ms']:.4f} ({c['faces']} "
                     f"faces), triangle_grid + unit normals {c['one_off']['triangle_grid_ms']:.4f}")
        for stride in (1, 4):
            s = c[f"stride {stride}"]
            lines.append(
                f"  stride {stride}, {s['points']} points\n"
                f"    pixel order:  fused {fmt(s, 'fused')}   plain torch {fmt(s, 'torch')}   "
                f"icp_sums on the mesh {fmt(s, 'mesh')}\n"
                f"    shuffled:     fused {fmt(s, 'fused shuffled')}   plain torch "
                f"{fmt(s, 'torch shuffled')}   icp_sums on the mesh {fmt(s, 'mesh shuffled')}\n"
                f"    refine_pose_tsdf {fmt(s, 'refine')}: {s['iterations']} iterations, converged "
                f"{s['converged']}, rank {s['rank']}, matched {s['matched']}, rmse "
                f"{s['first_rmse']:.3e} -> {s['rmse']:.3e}, ends {s['error_rad']:.2e} rad / "
                f"{s['error_units']:.2e} from the true pose; fused and torch sums agree to "
                f"{s['torch_rel_diff']:.1e} of the largest"
                + (f"\n    integrate_tsdf of the frame {fmt(s, 'integrate')}: a tracked frame costs "
                   f"refine + integrate" if "integrate" in s else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
