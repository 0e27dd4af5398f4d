"""Device time of mesh surface sampling (a record, not a gate): what
``ops.sample_mesh_surface`` costs on the analytic room's meshes of 466, 7 291 and
181 350 faces (steps 1, 0.25 and 0.05) at densities that give about 10^5 and
10^6 samples, how much of it each kernel is, and what a plain-torch sampler
takes.

  hip whole    ops.sample_mesh_surface without attributes: the count kernel,
               torch's int64 cumsum, the host read of the total that sizes the
               outputs, the sample kernel;
  hip labels   the same with the mesh's labels carried to the samples;
  hip counts   ucsa_face_sample_counts alone;
  hip samples  ucsa_mesh_surface_samples alone (no attributes) on that call's
               offsets: the per-lane binary search of ceil(log2(F + 1))
               dependent loads and the seven floats and one int per sample;
  torch        face areas by ``torch.linalg.cross``, ``torch.multinomial`` on
               them (with replacement), two ``torch.rand`` numbers per sample
               folded by ``u + v > 1``, the point from the gathered corners:
               binomial face counts, white-noise positions, another set in
               every call.

Before anything is timed the kernels alone must give the whole op's bytes.
``--lib`` loads another build of libucsa_hip.so, for the A/B of a kernel
variant; its outputs must equal the first build's bytes too (``--expect``).
All variants alternate in one process; device events after a warm-up; median /
best / worst ms.  One JSON line, then a table, both also written to --out.

    python tools/sample_time.py [--steps 1 0.25 0.05] [--samples 100000 1000000]
        [--rounds 9] [--out profiles/sample_time.txt] [--lib PATH] [--commit ID]
        [--parent ID]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.nearest_time import _time  # noqa: E402


def torch_sampler(V, Fc, n):
    tri = V[Fc.long()]                                                  # [F,3,3]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * torch.linalg.cross(e1, e2).norm(dim=1)
    f = torch.multinomial(area, n, replacement=True)
    uv = torch.rand((n, 2), device=V.device)
    uv = torch.where((uv.sum(1) > 1.0)[:, None], 1.0 - uv, uv)
    return tri[f, 0] + uv[:, :1] * e1[f] + uv[:, 1:] * e2[f], f


def raw_calls(V, Fc, res, seed):
    """the two kernels alone, on the offsets of ``res``"""
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    nv, nf, S = int(V.shape[0]), int(Fc.shape[0]), int(res["n_samples"])
    area, count = torch.empty_like(res["area"]), torch.empty_like(res["count"])
    pts, face, bary = (torch.empty_like(res[k]) for k in ("points", "face", "bary"))
    first = res["first"]

    def counts_():
        assert l.ucsa_face_sample_counts(p(V), nv, p(Fc), nf, res["density"], seed, p(area),
                                         p(count), None) == 0

    def samples_():
        assert l.ucsa_mesh_surface_samples(p(V), nv, p(Fc), nf, p(first), S, seed, None, None, None,
                                           p(pts), p(face), p(bary), None, None, None, None) == 0
    counts_()
    samples_()
    torch.cuda.synchronize()
    assert torch.equal(area.view(torch.int32), res["area"].view(torch.int32)), "counts: other bytes"
    assert torch.equal(count, res["count"]) and torch.equal(face, res["face"])
    assert torch.equal(pts.view(torch.int32), res["points"].view(torch.int32)), "samples: other bytes"
    assert torch.equal(bary.view(torch.int32), res["bary"].view(torch.int32))
    return counts_, samples_


def digest(res):
    h = hashlib.sha256()
    for k in ("points", "face", "bary", "labels", "area", "count", "first"):
        h.update(res[k].cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=float, nargs="+", default=[1.0, 0.25, 0.05])
    ap.add_argument("--samples", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_time.txt"))
    ap.add_argument("--lib", default=None, help="another build of libucsa_hip.so (A/B)")
    ap.add_argument("--expect", default=None,
                    help="a JSON line of an earlier run: the outputs must have its digests")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default="unknown")
    a = ap.parse_args()
    from ucsa_neural_rendering_amd import _lib
    if a.lib is not None:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from ucsa_neural_rendering_amd import ops
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    expect = None
    if a.expect is not None:
        with open(a.expect) as f:
            expect = json.loads(f.readline())["cases"]
    dev = "cuda"
    room = SyntheticRoom(0)
    rec = {"commit": a.commit, "parent": a.parent, "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "lib": "default" if a.lib is None else os.path.basename(a.lib),
           "cases": {}}
    for step in a.steps:
        m = room.labelled_mesh(step)
        V = torch.from_numpy(np.asarray(m["verts"], np.float32)).to(dev)
        Fc = torch.from_numpy(np.asarray(m["faces"], np.int32)).to(dev)
        L = torch.from_numpy(np.asarray(m["labels"]).astype(np.uint8)).to(dev)
        area = ops.sample_mesh_surface(V, Fc, 1.0, a.seed)["area"]
        total = float(np.sum(area.cpu().numpy(), dtype=np.float64))
        for n in a.samples:
            density = n / total
            res = ops.sample_mesh_surface(V, Fc, density, a.seed, labels=L)
            counts_, samples_ = raw_calls(V, Fc, res, a.seed)
            S = res["n_samples"]
            name = f"{int(Fc.shape[0])} faces, {n} samples"
            case = {"faces": int(Fc.shape[0]), "area": round(total, 4), "density": res["density"],
                    "n_samples": S, "largest_count": int(res["count"].max()),
                    "empty_faces": int((res["count"] == 0).sum()), "digest": digest(res)}
            if expect is not None:
                assert expect[name]["digest"] == case["digest"], f"{name}: other bytes"
                case["same_bytes_as"] = os.path.basename(a.expect)
            fns = {"hip whole": lambda: ops.sample_mesh_surface(V, Fc, density, a.seed),
                   "hip labels": lambda: ops.sample_mesh_surface(V, Fc, density, a.seed, labels=L),
                   "hip counts": counts_, "hip samples": samples_,
                   "torch": lambda: torch_sampler(V, Fc, S)}
            case.update(_time(fns, a.rounds))
            rec["cases"][name] = case
    out = [json.dumps(rec), "",
           f"mesh surface sampling, ms per call (median / best / worst of {a.rounds} alternated "
           f"rounds); commit {a.commit} (parent {a.parent}), {rec['device']}, library: {rec['lib']}",
           "hip whole / hip labels: ops.sample_mesh_surface without attributes / with labels, the "
           "host read of the total included; hip counts / hip samples: the kernels alone; torch: "
           "multinomial on the areas + random barycentrics"]
    for name, c in rec["cases"].items():
        out.append(f"{name}: area {c['area']}, density {c['density']:.2f}, {c['n_samples']} samples, "
                   f"largest count {c['largest_count']}, {c['empty_faces']} faces without a sample, "
                   f"sha256 of the outputs {c['digest']}"
                   + (f" (as in {c['same_bytes_as']})" if "same_bytes_as" in c else ""))
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
