"""Time of the lock-step ICP step and of a search that uses it (a record, not a gate).

The scene of tools/global_register_time.py: eight 480 x 640 views of a loop through
SyntheticRoom(0) integrated at their true poses into 128^3 over [-3.05, 3.05]^3
with trunc = 4 voxels; the points are those of a ninth view back-projected at
stride 4 in its camera frame (19 200 pixels), and a fixed subset of 2 069 of them.
The K transforms are that view's true pose moved by twists of up to 2 deg and
0.02 units: the points lie in the band, as they do in a loop's later iterations.

  (a) batch    one ops.register.tsdf_sums_batch call for K transforms
      single   K ops.register.tsdf_sums calls, one per transform, all of them
               timed (nothing is scaled); the rows of the two are compared
      Device events, alternated in one process after a warm-up; median / best.
  (b) meshes   a whole utils.registration.global_register_meshes call (the mesh of
               the volume against itself moved by a turn of more than 150 deg,
               2 048 samples, 4 096 rotations) with ``lockstep`` False and True,
               alternated, at keep 16 and keep 64: a host clock around a
               synchronise; and the part of it spent inside step 3, the
               refinement (the register_points_tsdf / register_points_tsdf_batch
               calls, which end in a blocking read).  The two results are compared.

    python tools/lockstep_time.py [--rounds 5] [--commit ID] [--out profiles/lockstep_time.txt]
One JSON line, then a table; both are also written to ``--out``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.register_time import time_fns  # noqa: E402
from tools.tsdf_register_time import FRAME, H, VIEWS, W, cast_depth  # noqa: E402

DIM, COUNTS, SIZES, KEEPS = 128, (1, 16, 64, 256), (2069, 19200), (16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep_time.txt"))
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, _slerp_loop_poses
    from ucsa_neural_rendering_amd.utils import registration as REG
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import extract_mesh
    room = SyntheticRoom(0).to("cuda")
    poses = _slerp_loop_poses(VIEWS + 1, seed=123).numpy().astype(np.float32)
    K4 = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    depth = torch.stack([cast_depth(room, poses[b], K4) for b in range(VIEWS + 1)]).contiguous()
    h = 6.1 / (DIM - 1)
    trunc = 4.0 * h
    vol = ops.tsdf_volume((DIM,) * 3, [-3.05] * 3, h, device="cuda")
    ops.integrate_tsdf(vol, depth[:VIEWS], torch.from_numpy(poses[:VIEWS]).cuda(), K4, trunc)
    pix = REG.backproject(depth[FRAME], K4, 4)
    gen = torch.Generator(device="cuda").manual_seed(0)
    order = torch.randperm(pix.shape[0], device="cuda", generator=gen)
    points = {n: (pix if n >= pix.shape[0] else pix[order[:n]].contiguous()) for n in SIZES}
    g = np.random.default_rng(7)
    pose = poses[FRAME].astype(np.float64)
    near = []
    for _ in range(max(COUNTS)):
        axis, shift = g.normal(size=3), g.normal(size=3)
        near.append(REG.compose(pose, np.concatenate(
            [np.radians(g.uniform(0, 2.0)) * axis / np.linalg.norm(axis),
             g.uniform(0, 0.02) * shift / np.linalg.norm(shift)])))
    near = np.stack(near)
    rec = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
           "volume": DIM, "step": {}, "meshes": {}}
    # (a) one batch call against K single calls
    for n, pts in points.items():
        for K in COUNTS:
            T = torch.from_numpy(near[:K, :3].astype(np.float32)).cuda()
            fns = {"batch": lambda: ops.register.tsdf_sums_batch(vol, pts, T, trunc),
                   "single": lambda: [ops.register.tsdf_sums(vol, pts, M, trunc)
                                      for M in near[:K]]}
            t = time_fns(fns, a.rounds)
            one = torch.stack(fns["single"]())
            got = fns["batch"]()
            rec["step"][f"K {K} N {int(pts.shape[0])}"] = {
                "batch": t["batch"], "single": t["single"],
                "matched_share": round(float(got[:, 28].mean()) / int(pts.shape[0]), 3),
                "rows_equal": bool(torch.equal(one.view(torch.int64), got.view(torch.int64)))}
            print(f"K {K} N {n}: done", file=sys.stderr, flush=True)
    # (b) a whole search with and without lock step
    mv, mf, _, _ = extract_mesh(vol, 1)
    dst = {"verts": mv.cpu().numpy(), "faces": mf.cpu().numpy()}
    g = np.random.default_rng(5003)
    axis = g.normal(size=3)
    M = REG.compose(np.eye(4), np.concatenate([g.uniform(np.radians(150.0), np.pi) * axis
                                               / np.linalg.norm(axis), g.uniform(-1, 1, 3)]))
    inv = np.linalg.inv(M)
    src = {"verts": (dst["verts"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3])
           .astype(np.float32), "faces": dst["faces"]}
    inside = [0.0]

    def clocked(fn):
        def run(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            inside[0] += 1e3 * (time.perf_counter() - t0)
            return out
        return run
    plain = (REG.register_points_tsdf, REG.register_points_tsdf_batch)
    REG.register_points_tsdf, REG.register_points_tsdf_batch = clocked(plain[0]), clocked(plain[1])
    try:
        for keep in KEEPS:
            whole, step3, outs = {False: [], True: []}, {False: [], True: []}, {}
            for r in range(1 + a.rounds):
                for lock in (False, True):
                    inside[0] = 0.0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    outs[lock] = REG.global_register_meshes(src, dst, h, samples=2048, keep=keep,
                                                            lockstep=lock)
                    torch.cuda.synchronize()
                    if r:                                         # the first round warms up
                        whole[lock].append(1e3 * (time.perf_counter() - t0))
                        step3[lock].append(inside[0])
            rot, trans = REG.transform_distance(outs[True]["transform"], M, np.zeros(3))
            same = outs[True]["transform"].tobytes() == outs[False]["transform"].tobytes() and \
                all(x["index"] == y["index"] and x["score"] == y["score"] and
                    x["transform"].tobytes() == y["transform"].tobytes()
                    for x, y in zip(outs[True]["candidates"], outs[False]["candidates"]))
            stat = lambda v: {"median_ms": round(float(np.median(v)), 2),
                              "best_ms": round(float(np.min(v)), 2)}
            rec["meshes"][f"keep {keep}"] = {
                "faces": int(mf.shape[0]), "points": outs[True]["n_points"],
                "sequential": {"whole": stat(whole[False]), "step3": stat(step3[False])},
                "lockstep": {"whole": stat(whole[True]), "step3": stat(step3[True])},
                "results_equal": bool(same), "error_rad": rot, "error_units": trans,
                "score": list(outs[True]["score"]),
                "winner_fine_iterations": outs[True]["iterations"]}
            print(f"keep {keep}: done", file=sys.stderr, flush=True)
    finally:
        REG.register_points_tsdf, REG.register_points_tsdf_batch = plain
    lines = [json.dumps(rec), "",
             f"lock-step ICP against a {DIM}^3 TSDF volume of {VIEWS} views, points of one 480 x 640 "
             f"frame at stride 4; ms median / best of {a.rounds}; commit {a.commit}, {rec['device']}",
             "  (a) one tsdf_sums_batch call against K tsdf_sums calls (device events, all K timed):"]
    for name, c in rec["step"].items():
        b, s = c["batch"], c["single"]
        lines.append(f"    {name}: batch {b['median_ms']:.4f} / {b['best_ms']:.4f}   K single calls "
                     f"{s['median_ms']:.4f} / {s['best_ms']:.4f}: {s['median_ms'] / b['median_ms']:.1f}x"
                     f"   matched share {c['matched_share']}, rows equal: {c['rows_equal']}")
    lines.append("  (b) global_register_meshes, the volume's mesh against itself moved, 2 048 samples, "
                 "4 096 rotations (host clock around a synchronise):")
    for name, m in rec["meshes"].items():
        q, l = m["sequential"], m["lockstep"]
        lines.append(
            f"    {name}, {m['points']} points: whole call sequential {q['whole']['median_ms']:.1f} / "
            f"{q['whole']['best_ms']:.1f}, lock step {l['whole']['median_ms']:.1f} / "
            f"{l['whole']['best_ms']:.1f}; inside step 3 (the refinement) sequential "
            f"{q['step3']['median_ms']:.1f} / {q['step3']['best_ms']:.1f}, lock step "
            f"{l['step3']['median_ms']:.1f} / {l['step3']['best_ms']:.1f}; results equal: "
            f"{m['results_equal']}; ends {m['error_rad']:.2e} rad / {m['error_units']:.2e} from the "
            f"move, score {m['score']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
