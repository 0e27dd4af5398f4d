"""Device time of the weighted ICP steps against the unweighted ones (a record, not
a gate).

The scene is tools/projective_time.py's: eight 480 x 640 views of a loop through
SyntheticRoom(0) integrated at their true poses into 128^3 over [-3.05, 3.05]^3
with trunc = 4 voxels; the frame is a ninth view under a pose 1 degree and 0.02
away from its own; the projective target is the model ray-cast from that pose.
Strides 1 and 4: 307 200 and 19 200 source points.

Per route (projective, tsdf) and stride the rows are

  plain         ops.register.projective_sums / tsdf_sums, the existing entry points
  none          the weighted entry point with kind "none" and no point weights
  huber, tukey  the weighted entry point with that kernel (scale 0.05)
  ... +p        the same three with a weight per point

A sample is ``--calls`` back-to-back calls between two device events, divided by
their number: one call is a few hundredths of a millisecond, too short a window
on its own.  All rows are alternated in one process after a warm-up of every
row; median / best of ``--rounds`` samples.

    python tools/robust_icp_time.py [--rounds 5] [--calls 50] [--commit ID]
        [--out profiles/robust_icp_time.txt]
One JSON line, then a table; both are also written to ``--out``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.tsdf_register_time import FRAME, VIEWS, H, W, cast_depth  # noqa: E402

N = 128
SCALE = 0.05


def time_windows(fns, rounds, calls):
    """median / best per-call ms of ``rounds`` windows of ``calls`` calls, alternated"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_icp_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("robust_icp_time.py measures on the GPU: none found")
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, _slerp_loop_poses
    from ucsa_neural_rendering_amd.utils import registration as REG
    room = SyntheticRoom(0).to("cuda")
    poses = _slerp_loop_poses(VIEWS + 1, seed=123).numpy().astype(np.float32)
    K = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    depth = torch.stack([cast_depth(room, poses[b], K) for b in range(VIEWS + 1)]).contiguous()
    pose = poses[FRAME].astype(np.float64)
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    start = REG.compose(pose, np.concatenate([np.radians(1.0) * axis, [0.012, -0.012, 0.0106]]))
    h = 6.1 / (N - 1)
    trunc = 4.0 * h
    vol = ops.tsdf_volume((N, N, N), [-3.05] * 3, h, device="cuda")
    ops.integrate_tsdf(vol, depth[:VIEWS], torch.from_numpy(poses[:VIEWS]).cuda(), K, trunc)
    frame = depth[FRAME]
    near, far, md, mc, reject = 0.05, 20.0, 0.3, 0.8, 12
    src = REG.frame_maps(frame, K, None, 1)[0]
    dst = REG.model_maps(vol, start, K, [(H, W)], trunc, near, far)[0]
    eye = np.eye(4)
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "calls": a.calls, "frame": [H, W], "views": VIEWS, "volume": N, "scale": SCALE,
           "cases": {}}
    R = ops.register
    for stride in (1, 4):
        sub_maps = {k: v[::stride, ::stride].contiguous() for k, v in src.items()
                    if torch.is_tensor(v)}
        pts, nrm = REG._source_rows(sub_maps, reject)
        world = REG.backproject(frame, K, stride)
        g = torch.Generator(device="cuda").manual_seed(stride)
        pw = {"projective": 0.1 + torch.rand(pts.shape[0], device="cuda", generator=g),
              "tsdf": 0.1 + torch.rand(world.shape[0], device="cuda", generator=g)}
        tgt = (dst["points"], dst["normals"], dst["mask"], K, eye, md, mc, reject)
        fns = {"projective plain": lambda: R.projective_sums(pts, nrm, *tgt),
               "tsdf plain": lambda: R.tsdf_sums(vol, world, start, trunc)}
        for kind in ("none", "huber", "tukey"):
            for tag, weights in (("", False), ("+p", True)):
                sc = None if kind == "none" else SCALE
                fns[f"projective {kind}{tag}"] = \
                    lambda kind=kind, sc=sc, w=weights: R.projective_sums_weighted(
                        pts, nrm, *tgt, pw["projective"] if w else None, kind, sc)
                fns[f"tsdf {kind}{tag}"] = \
                    lambda kind=kind, sc=sc, w=weights: R.tsdf_sums_weighted(
                        vol, world, start, trunc, 1.0, 1.0, pw["tsdf"] if w else None, kind, sc)
        sub = time_windows(fns, a.rounds, a.calls)
        counted = {k: float(fn().cpu().numpy()[28]) for k, fn in fns.items()}
        same = {route: bool(torch.equal(fns[f"{route} plain"]().view(torch.int64),
                                        fns[f"{route} none"]().view(torch.int64)))
                for route in ("projective", "tsdf")}
        rec["cases"][f"stride {stride}"] = {
            "points": {"projective": int(pts.shape[0]), "tsdf": int(world.shape[0])},
            "rows": sub, "counted": counted, "none_equals_plain_bit_for_bit": same}
    fmt = lambda c: f"{c['median_ms']:.4f} / {c['best_ms']:.4f}"
    lines = [json.dumps(rec), "",
             f"Weighted ICP steps, one {H} x {W} frame 1 deg / 0.02 off against {N}^3 fused from "
             f"{VIEWS} such views; ms per call, median / best of {a.rounds} windows of {a.calls} "
             f"calls; scale {SCALE}; commit {a.commit}, {rec['device']}"]
    for stride in (1, 4):
        s = rec["cases"][f"stride {stride}"]
        for route in ("projective", "tsdf"):
            lines.append(f"  stride {stride}, {route}, {s['points'][route]} points (kind none "
                         f"equals plain bit for bit: {s['none_equals_plain_bit_for_bit'][route]})")
            for name in ("plain", "none", "none+p", "huber", "huber+p", "tukey", "tukey+p"):
                key = f"{route} {name}"
                lines.append(f"    {name:8s} {fmt(s['rows'][key])}   rows counted "
                             f"{int(s['counted'][key])}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
