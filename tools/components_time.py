"""Device time of the connected-component labelling (a record, not a gate), so
that the next reader knows whether the tile-local LDS stage of
ucsa_voxel_components earns its place.

Lattice: room-like band masks (the walls, floor and ceiling of a box, three
voxels thick, the shells of a few boxes inside it, and specks in free space) at
n^3 for n in --sizes, at 6 and 26 connectivity:

  hip           ops.voxel_components (csrc/components.hip): tile labelling in
                LDS, unions across tile borders, flatten -- three launches;
  hip no-lds    the same entry with UCSA_COMPONENTS_NO_LDS=1: every union a
                global atomic (init, hook, flatten);
  torch         labels start as the voxel's index; a masked max_pool3d of the
                negated labels (float64: exact to 2^53), iterated until nothing
                changes, checked every 8 passes.  Timed up to --torch_max only
                (its pass count grows with the diameter of the components);
  sizes         ops.component_sizes of the labelling.

Mesh: the analytic room's mesh, ops.mesh_components against the same idea in
torch (scatter_reduce_ 'amin' over the directed edges until nothing changes).

The outputs of all forms are compared before anything is timed.  Alternated in
one process, device events after a warm-up; median / best ms.  One JSON line,
then a table.

    python tools/components_time.py [--sizes 128 256 512] [--torch_max 256] [--rounds 7]
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


def room_mask(n, dev, seed=0):
    g = np.random.default_rng(seed)
    m = torch.zeros(n, n, n, dtype=torch.bool, device=dev)

    def shell(lo, hi, t):
        box = torch.zeros_like(m)
        box[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        box[lo[0] + t:hi[0] - t, lo[1] + t:hi[1] - t, lo[2] + t:hi[2] - t] = False
        return box
    e = n // 16
    m |= shell((e, e, e), (n - e, n - e, n - e), 3)
    for _ in range(6):                                          # furniture
        size = g.integers(n // 10, n // 4, 3)
        lo = g.integers(2 * e, n - 2 * e - size)
        m |= shell(tuple(lo), tuple(lo + size), 2)
    for _ in range(40):                                         # floaters
        c = g.integers(2 * e, n - 2 * e, 3)
        m[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 3] = True
    return m


def torch_lattice(mask, connectivity):
    import torch.nn.functional as F
    n = mask.numel()
    idx = torch.arange(n, dtype=torch.float64, device=mask.device).view(mask.shape)
    ninf = torch.full_like(idx, float("-inf"))
    lab = torch.where(mask, -idx, ninf)
    passes = 0
    while True:
        before = lab
        for _ in range(8):
            x = lab[None, None]
            if connectivity == 26:
                pooled = F.max_pool3d(x, 3, 1, 1)
            else:
                pooled = torch.maximum(torch.maximum(F.max_pool3d(x, (3, 1, 1), 1, (1, 0, 0)),
                                                     F.max_pool3d(x, (1, 3, 1), 1, (0, 1, 0))),
                                       F.max_pool3d(x, (1, 1, 3), 1, (0, 0, 1)))
            lab = torch.where(mask, pooled[0, 0], ninf)
        passes += 8
        if torch.equal(lab, before):
            break
    return torch.where(mask, -lab, torch.ones_like(lab).neg()).to(torch.int32), passes


def torch_graph(adj):
    off, nbr = adj[0].long(), adj[1].long()
    V = off.numel() - 1
    src = torch.repeat_interleave(torch.arange(V, device=off.device), torch.diff(off))
    lab = torch.arange(V, device=off.device)
    passes = 0
    while True:
        before = lab
        for _ in range(8):
            lab = lab.clone().scatter_reduce_(0, src, lab[nbr], "amin")
        passes += 8
        if torch.equal(lab, before):
            break
    return lab.to(torch.int32), passes


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
    return {k: {"median_ms": round(float(np.median(v)), 4), "best": round(float(np.min(v)), 4)}
            for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--torch_max", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    dev = "cuda"

    def hip(mask, c, no_lds):
        # the library reads the switch once per process: re-read it around the call
        if no_lds:
            os.environ["UCSA_COMPONENTS_NO_LDS"] = "1"
        else:
            os.environ.pop("UCSA_COMPONENTS_NO_LDS", None)
        ops.env_reload()
        return ops.voxel_components(mask, c)

    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "cases": {}, "mesh": {}}
    for n in a.sizes:
        mask = room_mask(n, dev)
        for c in (6, 26):
            fns = {"hip": lambda c=c: hip(mask, c, False),
                   "hip no-lds": lambda c=c: hip(mask, c, True)}
            lab = fns["hip"]()
            assert torch.equal(lab, fns["hip no-lds"]())
            case = {"n": n, "set": round(float(mask.float().mean()), 4),
                    "components": int((lab.view(-1) == torch.arange(
                        lab.numel(), dtype=torch.int32, device=dev)).sum())}
            slow = {}
            if n <= a.torch_max:
                want, passes = torch_lattice(mask, c)
                assert torch.equal(lab, want), (n, c)
                case["torch_passes"] = passes
                slow = _time({"torch": lambda c=c: torch_lattice(mask, c)}, 1)
            fns["sizes"] = lambda: ops.component_sizes(lab)
            case.update(_time(fns, a.rounds))
            case.update(slow)
            rec["cases"][f"{n}^3 connectivity {c}"] = case
        del mask
        torch.cuda.empty_cache()
    os.environ.pop("UCSA_COMPONENTS_NO_LDS", None)
    ops.env_reload()
    room = SyntheticRoom(0).labelled_mesh(0.02)
    faces = torch.from_numpy(np.ascontiguousarray(room["faces"], np.int32)).to(dev)
    V = int(np.asarray(room["verts"]).shape[0])
    adj = ops.mesh_adjacency(faces, V)
    got = ops.mesh_components(adj)
    want, passes = torch_graph(adj)
    assert torch.equal(got, want)
    rec["mesh"] = {"V": V, "E": int(adj[1].numel()), "components": int(torch.unique(got).numel()),
                   "torch_passes": passes}
    rec["mesh"].update(_time({"mesh hip": lambda: ops.mesh_components(adj)}, a.rounds))
    rec["mesh"].update(_time({"mesh torch": lambda: torch_graph(adj)}, 1))
    print(json.dumps(rec))
    print(f"\nconnected components, ms per call (median / best of {a.rounds}; the torch forms "
          f"once); commit {a.commit} (parent {a.parent}), {rec['device']}")
    for name, c in rec["cases"].items():
        print(f"{name} (set {c['set']}, {c['components']} components"
              + (f", torch: {c['torch_passes']} passes" if "torch_passes" in c else "") + ")")
        for k in ("hip", "hip no-lds", "sizes", "torch"):
            if k in c:
                print(f"    {k:<12} {c[k]['median_ms']:.4f} / {c[k]['best']:.4f}")
    m = rec["mesh"]
    print(f"mesh, {m['V']} vertices, {m['E']} directed edges, {m['components']} components "
          f"(torch: {m['torch_passes']} passes)")
    for k in ("mesh hip", "mesh torch"):
        print(f"    {k:<12} {m[k]['median_ms']:.4f} / {m[k]['best']:.4f}")


if __name__ == "__main__":
    main()
