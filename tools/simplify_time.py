"""Device time of mesh simplification by vertex clustering (a record, not a
gate): what ``ops.simplify_mesh`` costs on the analytic room's meshes at step
0.05 and 0.02 with cells of 2, 5 and 10 times the step, how much of it is the
reduce kernel, and what a plain-torch form of the same clustering takes.

  hip whole    ops.simplify_mesh with the mesh's labels: keys, torch's stable
               sort and unique, the reduce, the face kernel, the face
               de-duplication and compaction, with the host reads that size the
               outputs;
  hip reduce   ucsa_cluster_reduce alone on the sorted order of that call;
  hip faces    ucsa_cluster_faces alone;
  torch        cells by floor((v - origin) / cell), ``torch.unique`` of the linear
               cell index with the inverse, and float ``index_add_`` means of
               the positions: the vertex part only, no labels, no faces, and
               sums whose order the device chooses (not reproducible to the
               bit);
  one cell     the whole op and the reduce alone with a cell larger than the
               room: one lane walks every vertex, the documented worst case.

Before anything is timed the kernels alone must give the whole op's bytes, and
the share of vertices whose torch mean differs from the kernel's by more than
1e-3 of the cell is recorded (the clusters are the same wherever the cell of a
vertex is not decided by the last bit of a division; a plain sum of coordinates
is itself off by about 1e-5).  All variants alternate in one process; device events after a
warm-up; median / best / worst ms.  One JSON line, then a table, both also
written to --out.

    python tools/simplify_time.py [--steps 0.05 0.02] [--factors 2 5 10] [--rounds 7]
        [--out profiles/simplify_time.txt] [--commit ID] [--parent ID]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.nearest_time import _time  # noqa: E402


def torch_means(V, cell, dims):
    lo = V.min(0).values
    # a tensor divisor: a Python scalar would be turned into a multiplication by 1 / cell,
    # which puts vertices that lie on a cell wall (the room's lattice) into other cells
    idx = torch.floor((V - lo) / torch.full((1, 3), cell, dtype=V.dtype, device=V.device)).long()
    # the grid's clamp: what rounding puts on the far wall belongs to the last cell
    idx = torch.minimum(idx, torch.tensor([d - 1 for d in dims], device=V.device))
    lin = (idx[:, 0] * dims[1] + idx[:, 1]) * dims[2] + idx[:, 2]
    _, inv, counts = torch.unique(lin, return_inverse=True, return_counts=True)
    s = torch.zeros((counts.numel(), 3), dtype=torch.float32, device=V.device)
    s.index_add_(0, inv, V)
    return s / counts[:, None].float(), inv


def raw_calls(ops, V, Fc, L, res, split=False):
    """the reduce and the face kernel alone, on what ops.simplify_mesh sorted"""
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    n, nf, K = int(V.shape[0]), int(Fc.shape[0]), int(res["verts"].shape[0])
    keys = torch.empty(n, dtype=torch.int64, device=V.device)
    assert l.ucsa_vertex_cluster_keys(p(V), n, (C.c_float * 3)(*res["origin"]), res["cell"],
                                      (C.c_uint32 * 3)(*res["dims"]), p(L), p(keys), None) == 0
    order = torch.sort(keys, stable=True).indices.to(torch.int32)
    first = torch.zeros(K + 1, dtype=torch.int32, device=V.device)
    first[1:] = torch.cumsum(res["count"], 0)
    ov, ol = torch.empty_like(res["verts"]), torch.empty_like(res["labels"])
    oc = torch.empty_like(res["count"])
    tri = torch.empty((nf, 3), dtype=torch.int32, device=V.device)
    keep = torch.empty(nf, dtype=torch.uint8, device=V.device)
    vm = res["vertex_map"]

    def reduce_():
        assert l.ucsa_cluster_reduce(p(V), None, None, p(L), n, p(order), p(first), K, p(ov), None,
                                     None, p(ol), p(oc), None) == 0

    def faces_():
        assert l.ucsa_cluster_faces(p(Fc), nf, p(vm), n, p(tri), p(keep), None) == 0
    reduce_()
    torch.cuda.synchronize()
    assert torch.equal(ov.view(torch.int32), res["verts"].view(torch.int32)), "reduce: other bytes"
    assert torch.equal(ol, res["labels"]) and torch.equal(oc, res["count"])
    return reduce_, faces_


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[0.05, 0.02])
    ap.add_argument("--factors", type=float, nargs="+", default=[2.0, 5.0, 10.0])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_time.txt"))
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    dev = "cuda"
    room = SyntheticRoom(0)
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "cases": {}}
    for step in a.steps:
        m = room.labelled_mesh(step)
        V = torch.from_numpy(np.asarray(m["verts"], np.float32)).to(dev)
        Fc = torch.from_numpy(np.asarray(m["faces"], np.int32)).to(dev)
        L = torch.from_numpy(np.asarray(m["labels"]).astype(np.uint8)).to(dev)
        for k in list(a.factors) + [None]:
            cell = 100.0 if k is None else step * k
            res = ops.simplify_mesh(V, Fc, cell, labels=L)
            reduce_, faces_ = raw_calls(ops, V, Fc, L, res)
            fns = {"hip whole": lambda: ops.simplify_mesh(V, Fc, cell, labels=L),
                   "hip reduce": reduce_, "hip faces": faces_}
            case = {"verts": [int(V.shape[0]), int(res["verts"].shape[0])],
                    "faces": [int(Fc.shape[0]), int(res["faces"].shape[0])], "cell": res["cell"],
                    "dims": list(res["dims"]), "largest_cluster": int(res["count"].max()),
                    "degenerate": res["degenerate"], "duplicate": res["duplicate"]}
            if k is not None:
                tm, inv = torch_means(V, res["cell"], res["dims"])
                mine = res["verts"][res["vertex_map"].long()]
                far = ((tm[inv] - mine).abs().max(1).values > 1e-3 * res["cell"]).float().mean()
                case["torch_clusters"] = int(tm.shape[0])
                case["torch_far"] = round(float(far), 6)
                fns["torch"] = lambda: torch_means(V, res["cell"], res["dims"])
            case.update(_time(fns, a.rounds if k is not None else min(a.rounds, 3)))
            name = f"step {step:g}, " + ("one cell" if k is None else f"cell x{k:g}")
            rec["cases"][name] = case
    out = [json.dumps(rec), "",
           f"mesh simplification by vertex clustering, ms per call (median / best / worst of "
           f"{a.rounds} alternated rounds, 3 for one cell); commit {a.commit} (parent {a.parent}), "
           f"{rec['device']}",
           "hip whole: ops.simplify_mesh with labels, host reads included; hip reduce / hip faces: "
           "the kernels alone; torch: unique + float index_add_ means of the positions only; one "
           "cell: every vertex in one cluster, one lane walks them all"]
    for name, c in rec["cases"].items():
        out.append(f"{name}: cell {c['cell']:.4f}, dims {c['dims']}, vertices {c['verts'][0]} -> "
                   f"{c['verts'][1]}, faces {c['faces'][0]} -> {c['faces'][1]} ({c['degenerate']} "
                   f"degenerate, {c['duplicate']} duplicate), largest cluster {c['largest_cluster']}"
                   + (f"; torch: {c['torch_clusters']} clusters, {c['torch_far']} of the vertices "
                      "with another mean" if "torch_far" in c else ""))
        for k, v in c.items():
            if isinstance(v, dict) and "median_ms" in v:
                out.append(f"    {k:<12} {v['median_ms']:.4f} / {v['best']:.4f} / {v['worst']:.4f}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
