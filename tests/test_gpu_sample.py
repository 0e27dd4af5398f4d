"""GPU: area-uniform sample points on a mesh (csrc/mesh_sample.hip:
ucsa_face_sample_counts, ucsa_mesh_surface_samples; ops.sample_mesh_surface)
against the plain loops of tests/sample_numpy.py, byte for byte, on the cases of
tests/test_sample_cpu.py: no face, one face with 0, 1, 65 and 5000 samples, 257
samples, runs of faces without a sample, invalid faces, a mesh 1e4 from the
origin, every subset of the attributes.  Guard words, unchanged inputs, a
malformed ``first``, argument codes; then the utilities of utils/mesh_eval.py
and scripts/score_mesh_3d.py on the analytic room: a hole in the middle of a
wall costs recall only when the query points are sampled from the surface."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from tests import sample_numpy as SP
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded
from tests.test_sample_cpu import ATTRS, NAMES, ONE_FACE, all_cases, want
from tests.test_surface_cpu import room

pytestmark = pytest.mark.gpu
F = np.float32
ARRAYS = ("points", "face", "bary", "normals", "rgb", "labels", "area", "count", "first")
DTYPES = {"points": torch.float32, "face": torch.int32, "bary": torch.float32,
          "normals": torch.float32, "rgb": torch.uint8, "labels": torch.uint8,
          "area": torch.float32, "count": torch.int32, "first": torch.int32}


def gpu_sample(c, use=ATTRS, **kw):
    opt = {k: _cu(c[k]) for k in use}
    kw.setdefault("seed", c["seed"])
    return _ops().sample_mesh_surface(_cu(c["verts"]).view(-1, 3), _cu(c["faces"]).view(-1, 3),
                                      kw.pop("density", c["density"]), **opt, **kw)


def assert_same(got, ref, use, tag):
    for k in ARRAYS:
        if k in ATTRS and k not in use:
            assert k not in got, (tag, k)
            continue
        assert got[k].dtype == DTYPES[k] and tuple(got[k].shape) == ref[k].shape, (tag, k)
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), (tag, k)
    assert got["n_samples"] == ref["n_samples"] and got["density"] == ref["density"], tag
    assert sorted(got) == sorted([k for k in ARRAYS if k not in ATTRS or k in use] +
                                 ["n_samples", "density"]), tag


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_restatement(name):
    assert_same(gpu_sample(all_cases()[name]), want(name), ATTRS, name)


def test_every_subset_of_the_attributes_and_integer_label_dtypes():
    for name in ("random", "zeros"):
        c, ref = all_cases()[name], want(name)
        for n in range(3):
            for use in itertools.combinations(ATTRS, n):
                assert_same(gpu_sample(c, use), ref, use, (name, use))
        for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
            got = _ops().sample_mesh_surface(_cu(c["verts"]), _cu(c["faces"]), c["density"],
                                             c["seed"], labels=_cu(c["labels"]).to(dt))
            assert_same(got, ref, ("labels",), (name, dt))


def test_a_higher_density_appends_to_every_face():
    c, lo = all_cases()["random"], want("random")
    hi = gpu_sample(c, density=2.5 * c["density"])
    first, count = hi["first"].cpu().numpy(), hi["count"].cpu().numpy()
    assert (count >= lo["count"]).all() and hi["n_samples"] > 2 * lo["n_samples"]
    rows = np.concatenate([first[f] + np.arange(lo["count"][f]) for f in range(count.size)])
    for k in ("points", "bary") + ATTRS:
        assert hi[k].cpu().numpy()[rows].tobytes() == lo[k].tobytes(), k


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_guard_words_unchanged_inputs_and_a_malformed_first():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    for name in ("one_65", "one_5000", "s257", "zeros", "invalid"):
        c, ref = all_cases()[name], want(name)
        nv, nf, S = c["verts"].shape[0], c["faces"].shape[0], ref["n_samples"]
        lab8 = c["labels"].astype(np.uint8)
        V, Fc, N, R, L = _cu(c["verts"]), _cu(c["faces"]), _cu(c["normals"]), _cu(c["rgb"]), _cu(lab8)
        area, c1 = guarded((nf,), torch.float32, -5.0)
        count, c2 = guarded((nf,), torch.int32, -5)
        assert l.ucsa_face_sample_counts(_p(V), nv, _p(Fc), nf, c["density"], c["seed"], _p(area),
                                         _p(count), None) == 0
        torch.cuda.synchronize()
        c1()
        c2()
        assert area.cpu().numpy().tobytes() == ref["area"].tobytes(), name
        assert count.cpu().numpy().tobytes() == ref["count"].tobytes(), name
        outs = {"points": guarded((S, 3), torch.float32, -5.0), "face": guarded((S,), torch.int32, -5),
                "bary": guarded((S, 3), torch.float32, -5.0),
                "normals": guarded((S, 3), torch.float32, -5.0),
                "rgb": guarded((S, 3), torch.uint8, 9), "labels": guarded((S,), torch.uint8, 9)}
        first = _cu(ref["first"])

        def run(first_):
            rc = l.ucsa_mesh_surface_samples(_p(V), nv, _p(Fc), nf, _p(first_), S, c["seed"], _p(N),
                                             _p(R), _p(L), *[_p(outs[k][0]) for k in outs], None)
            torch.cuda.synchronize()
            for _, ch in outs.values():
                ch()
            return rc
        assert run(first) == 0
        for k, (t, _) in outs.items():
            assert t.cpu().numpy().tobytes() == ref[k].tobytes(), (name, k)
        # malformed offsets: negative, decreasing, beyond S, all alike; the search is bounded and
        # every index clamped, and the restatement follows the same steps
        g = np.random.default_rng(41)
        bads = [ref["first"][::-1].copy(), np.full(nf + 1, -7, np.int32),
                np.full(nf + 1, 2 ** 31 - 1, np.int32), np.zeros(nf + 1, np.int32),
                g.integers(-2 ** 31, 2 ** 31, nf + 1).astype(np.int32),
                g.integers(-S - 5, 2 * S + 5, nf + 1).astype(np.int32)]
        for bad in bads[:6 if S <= 300 else 2]:
            assert run(_cu(bad)) == 0
            model = SP.mesh_surface_samples(c["verts"], c["faces"], bad, S, c["seed"], c["normals"],
                                            c["rgb"], lab8)
            for k, (t, _) in outs.items():
                assert t.cpu().numpy().tobytes() == model[k].tobytes(), (name, k)
        # the wrapper leaves its inputs alone as well
        _ops().sample_mesh_surface(V, Fc, c["density"], c["seed"], normals=N, rgb=R, labels=L)
        for t, a in ((V, c["verts"]), (Fc, c["faces"]), (N, c["normals"]), (R, c["rgb"]), (L, lab8),
                     (first, ref["first"])):
            assert t.cpu().numpy().tobytes() == a.tobytes(), name


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops, l = _ops(), _lib.lib()
    c, ref = all_cases()["random"], want("random")
    nv, nf, S = c["verts"].shape[0], c["faces"].shape[0], ref["n_samples"]
    V, Fc, N, R = _cu(c["verts"]), _cu(c["faces"]), _cu(c["normals"]), _cu(c["rgb"])
    L, first = _cu(c["labels"].astype(np.uint8)), _cu(ref["first"])
    nan, inf = float("nan"), float("inf")
    area, ca = guarded((nf,), torch.float32, 99.0)
    count, cc = guarded((nf,), torch.int32, 99)
    outs = [guarded((S, 3), torch.float32, 99.0), guarded((S,), torch.int32, 99),
            guarded((S, 3), torch.float32, 99.0), guarded((S, 3), torch.float32, 99.0),
            guarded((S, 3), torch.uint8, 99), guarded((S,), torch.uint8, 99)]
    op, of, ob, on, oc, ol = (t for t, _ in outs)

    def ccall(v=V, nv_=nv, f=Fc, nf_=nf, d=c["density"], a=area, n=count):
        return l.ucsa_face_sample_counts(_p(v), nv_, _p(f), nf_, d, 7, _p(a), _p(n), None)

    def scall(v=V, nv_=nv, f=Fc, nf_=nf, fi=first, s=S, nr=N, rg=R, lb=L, p=op, fa=of, b=ob, n=on,
              r=oc, la=ol):
        return l.ucsa_mesh_surface_samples(_p(v), nv_, _p(f), nf_, _p(fi), s, 7, _p(nr), _p(rg),
                                           _p(lb), _p(p), _p(fa), _p(b), _p(n), _p(r), _p(la), None)
    for rc, arg in ((ccall(v=None), 0), (ccall(nv_=2 ** 31), 1), (ccall(f=None), 2),
                    (ccall(nf_=2 ** 31), 3), (ccall(d=0.0), 4), (ccall(d=-1.0), 4),
                    (ccall(d=nan), 4), (ccall(d=inf), 4), (ccall(a=None), 6), (ccall(n=None), 7),
                    (scall(v=None), 0), (scall(nv_=2 ** 31), 1), (scall(f=None), 2),
                    (scall(nf_=2 ** 31), 3), (scall(nf_=0), 3), (scall(fi=None), 4),
                    (scall(s=2 ** 31), 5), (scall(p=None), 10), (scall(fa=None), 11),
                    (scall(b=None), 12), (scall(n=None), 13), (scall(r=None), 14),
                    (scall(la=None), 15)):
        assert rc == -(1000 + arg), (rc, arg)
    # legal: nothing to do, nothing launched
    assert ccall(v=None, f=None, nf_=0, a=None, n=None) == 0
    assert scall(v=None, f=None, fi=None, s=0, p=None, fa=None, b=None, n=None, r=None, la=None) == 0
    assert scall(nf_=0, s=0) == 0
    torch.cuda.synchronize()
    for t in (area, count, op, of, ob, on, oc, ol):
        assert (t == 99).all()                                # an argument error launches nothing
    # absent attributes need no output and leave it alone; no vertices: no face counts
    assert scall(nr=None, rg=None, lb=None, n=None, r=None, la=None) == 0
    assert ccall(v=None, nv_=0) == 0
    torch.cuda.synchronize()
    for ch in [ca, cc] + [x for _, x in outs]:
        ch()
    assert (on == 99).all() and (oc == 99).all() and (ol == 99).all()
    assert op.cpu().numpy().tobytes() == ref["points"].tobytes()
    assert (area == 0).all() and (count == 0).all()
    lab64 = _cu(c["labels"].astype(np.int64))
    d = c["density"]
    for bad in (lambda: ops.sample_mesh_surface(V.cpu(), Fc, d),
                lambda: ops.sample_mesh_surface(V, Fc.cpu(), d),
                lambda: ops.sample_mesh_surface(V, Fc.long(), d),
                lambda: ops.sample_mesh_surface(V, Fc[:, :2], d),
                lambda: ops.sample_mesh_surface(V[:, :2], Fc, d),
                lambda: ops.sample_mesh_surface(V, Fc, 0.0), lambda: ops.sample_mesh_surface(V, Fc, -1.0),
                lambda: ops.sample_mesh_surface(V, Fc, nan), lambda: ops.sample_mesh_surface(V, Fc, inf),
                lambda: ops.sample_mesh_surface(V, Fc, 1e39), lambda: ops.sample_mesh_surface(V, Fc, 1e-50),
                lambda: ops.sample_mesh_surface(V, Fc, "dense"),
                lambda: ops.sample_mesh_surface(V, Fc, d, seed=-1),
                lambda: ops.sample_mesh_surface(V, Fc, d, seed=2 ** 32),
                lambda: ops.sample_mesh_surface(V, Fc, d, seed=0.5),
                lambda: ops.sample_mesh_surface(V, Fc, d, max_samples=-1),
                lambda: ops.sample_mesh_surface(V, Fc, d, labels=lab64 - 1),
                lambda: ops.sample_mesh_surface(V, Fc, d, labels=lab64 + 251),
                lambda: ops.sample_mesh_surface(V, Fc, d, labels=lab64.float()),
                lambda: ops.sample_mesh_surface(V, Fc, d, labels=lab64.cpu()),
                lambda: ops.sample_mesh_surface(V, Fc, d, labels=lab64[:-1]),
                lambda: ops.sample_mesh_surface(V, Fc, d, normals=N.cpu()),
                lambda: ops.sample_mesh_surface(V, Fc, d, normals=N[:-1]),
                lambda: ops.sample_mesh_surface(V, Fc, d, rgb=R.cpu()),
                lambda: ops.sample_mesh_surface(V, Fc, d, rgb=R.float())):
        with pytest.raises(UcsaError):
            bad()
    # too many samples: refused before anything of that size exists
    with pytest.raises(UcsaError, match="lower density"):
        ops.sample_mesh_surface(V, Fc, d, max_samples=S - 1)
    assert ops.sample_mesh_surface(V, Fc, d, seed=c["seed"], max_samples=S)["n_samples"] == S
    one_v, one_f = _cu(ONE_FACE[0]), _cu(ONE_FACE[1])
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(UcsaError, match="lower density"):
        ops.sample_mesh_surface(one_v, one_f, 1e30, max_samples=10 ** 6)   # 2^24 of one face
    with pytest.raises(UcsaError, match="lower density"):
        ops.sample_mesh_surface(one_v.repeat(200, 1), (one_f + 3 * torch.arange(
            200, dtype=torch.int32, device="cuda")[:, None]), 1e30, max_samples=2 ** 40)
    assert torch.cuda.max_memory_allocated() - before < (1 << 20)


# ---- the utilities and the script on the analytic room -------------------------
THRESHOLD, MAX_DIST, DENSITY, HOLE_FACE, HOLE_R = 0.01, 0.2, 1000.0, 1, 0.28


@pytest.fixture(scope="module")
def hole():
    """The fine mesh of the room with the faces inside a disc of radius 0.28 in
    the middle of a wall removed.  The disc lies strictly inside ground-truth
    face 1, a right triangle with legs 1 on the wall x = -3 (inradius 0.2929)."""
    m = room()
    gt, fine = m["coarse"], m["fine"]
    gv, gf = gt["verts"].astype(F), gt["faces"].astype(np.int32)
    fv, ff = fine["verts"].astype(F), fine["faces"].astype(np.int32)
    t = gv[gf[HOLE_FACE]].astype(np.float64)
    side = [np.linalg.norm(t[1] - t[2]), np.linalg.norm(t[0] - t[2]), np.linalg.norm(t[0] - t[1])]
    centre = (side[0] * t[0] + side[1] * t[1] + side[2] * t[2]) / sum(side)
    assert gt["face_classes"][HOLE_FACE] == 0 and (t[:, 0] == -3.0).all()
    assert abs(0.5 * np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) - 0.5) < 1e-12
    dist = np.linalg.norm(fv.astype(np.float64) - centre, axis=1)
    gone = (dist[ff] <= HOLE_R).all(1)
    # nothing but the wall near the disc, and the wall's faces cover it
    assert (fv[dist <= HOLE_R + 0.15, 0] == -3.0).all()
    tri = fv[ff[gone]].astype(np.float64)
    edge = max(np.linalg.norm(tri[:, a] - tri[:, b], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    cut = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1).sum()
    assert edge < 0.0708 and np.pi * (HOLE_R - edge) ** 2 <= cut <= np.pi * HOLE_R ** 2
    return {"gv": gv, "gf": gf, "fv": fv, "ff": ff, "holed": ff[~gone], "centre": centre,
            "edge": float(edge)}


def test_a_hole_in_a_wall_costs_recall_only_when_the_surface_is_sampled(hole):
    """Every point of the disc of radius r - edge (edge: the longest edge of a
    removed face) lies in a removed face, so a ground-truth sample within
    r - edge - threshold of the centre is farther than the threshold from what
    is left and is lost; a sample farther than r from the centre lies on a face
    that stayed.  Both are counted on the samples themselves: an exact bracket.
    The disc's share of the area then brackets the same count: the face's count
    is within 1 of area * density, and the points inside the disc are allowed a
    binomial sampler's five deviations (the set's discrepancy is far smaller,
    tests/test_sample_cpu.py); the total is within 2.5 sqrt(F) of sum(area) *
    density."""
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance
    h = hole
    args = (h["fv"], h["gv"], THRESHOLD, MAX_DIST)
    intact = mesh_distance(*args, pred_faces=h["ff"], gt_faces=h["gf"])
    holed = mesh_distance(*args, pred_faces=h["holed"], gt_faces=h["gf"])
    assert "sampled" not in intact and intact["recall"] == holed["recall"]   # the corners see nothing
    s_intact = mesh_distance(*args, pred_faces=h["ff"], gt_faces=h["gf"], sample_density=DENSITY)
    s_holed = mesh_distance(*args, pred_faces=h["holed"], gt_faces=h["gf"], sample_density=DENSITY)
    res = _ops().sample_mesh_surface(_cu(h["gv"]), _cu(h["gf"]), DENSITY)
    n_gt, nf = res["n_samples"], h["gf"].shape[0]
    assert s_intact["sampled"][1] == s_holed["sampled"][1] == n_gt and s_intact["surface"] == (True, True)
    assert s_intact["sampled"][0] > 0 and s_holed["sampled"][0] > 0
    area = res["area"].cpu().numpy().astype(np.float64)
    total = float(area.sum())
    assert abs(n_gt - total * DENSITY) <= 2.5 * np.sqrt(nf) + 1e-6 * total * DENSITY
    lost = (s_intact["recall"] - s_holed["recall"]) * n_gt
    assert abs(lost - round(lost)) < 1e-6 * n_gt * 1e-3 + 1e-6
    lost = int(round(lost))
    d = np.linalg.norm(res["points"].cpu().numpy().astype(np.float64) - h["centre"], axis=1)
    r_in = HOLE_R - h["edge"] - THRESHOLD
    n_in, n_out = int((d <= r_in - 1e-5).sum()), int((d <= HOLE_R + 1e-5).sum())
    face = res["face"].cpu().numpy()
    assert (face[d <= HOLE_R + 1e-5] == HOLE_FACE).all()             # strictly inside one face
    n_face = int(res["count"][HOLE_FACE])
    assert abs(n_face - area[HOLE_FACE] * DENSITY) <= 1.0 + 1e-3
    margin = lambda p: 1.0 + 5.0 * np.sqrt(n_face * p * (1.0 - p))
    p_in, p_out = np.pi * r_in ** 2 / area[HOLE_FACE], np.pi * HOLE_R ** 2 / area[HOLE_FACE]
    print("recall", s_intact["recall"], "->", s_holed["recall"], "of", n_gt, "samples: lost", lost,
          "| samples within", r_in, "and", HOLE_R, "of the centre:", n_in, n_out,
          "| by area:", p_in * n_face, p_out * n_face, "| the disc's share", np.pi * HOLE_R ** 2 / total)
    assert 0 < n_in <= lost <= n_out
    assert p_in * n_face - margin(p_in) <= lost <= p_out * n_face + margin(p_out)
    assert s_holed["completeness"] > s_intact["completeness"]


def test_labels_are_scored_at_surface_samples_by_area():
    from ucsa_neural_rendering_amd.utils.mesh_eval import (_score, sample_surface, score_labels_3d,
                                                           score_voxel_labels_3d, transfer_labels)
    m = room()
    gt, fine = m["coarse"], m["fine"]
    c, ref = all_cases()["room"], want("room")
    pts, lab, res = sample_surface(gt["verts"], gt["faces"], c["density"], c["seed"], gt["labels"])
    assert pts.cpu().numpy().tobytes() == ref["points"].tobytes() and lab.dtype == torch.int32
    assert np.array_equal(lab.cpu().numpy(), ref["labels"]) and res["n_samples"] == ref["n_samples"]
    kw = dict(gt_faces=gt["faces"], sample_density=c["density"], seed=c["seed"])
    s = score_labels_3d(fine["verts"], fine["labels"], gt["verts"], gt["labels"], MAX_DIST, **kw)
    pred, index = transfer_labels(fine["verts"], fine["labels"], ref["points"], MAX_DIST,
                                  return_match=True)[:2]
    assert s == {**_score(pred, index, ref["labels"].astype(np.int32), 40), "sampled": ref["n_samples"]}
    scored = int(((ref["labels"] >= 1) & (ref["labels"] <= 40)).sum())
    assert s["vertices"] == scored > 0.9 * ref["n_samples"] and s["total_acc"] > 0.9
    surf = score_labels_3d(fine["verts"], fine["labels"], gt["verts"], gt["labels"], MAX_DIST,
                           pred_faces=fine["faces"], **kw)
    assert surf["sampled"] == ref["n_samples"] and surf["total_acc"] > 0.9
    plain = score_labels_3d(fine["verts"], fine["labels"], gt["verts"], gt["labels"], MAX_DIST)
    assert "sampled" not in plain and plain["vertices"] <= gt["verts"].shape[0]
    # about N samples; the voxel score passes the keywords through
    _, _, by_n = sample_surface(gt["verts"], gt["faces"], None, samples=20000)
    total = float(np.sum(ref["area"], dtype=np.float64))
    assert by_n["density"] == float(F(20000 / total))
    assert abs(by_n["n_samples"] - 20000) <= 2.5 * np.sqrt(gt["faces"].shape[0]) + 1
    with pytest.raises(ValueError):
        score_labels_3d(fine["verts"], fine["labels"], gt["verts"], gt["labels"], MAX_DIST,
                        sample_density=10.0)
    with pytest.raises(ValueError):
        sample_surface(gt["verts"], gt["faces"], 10.0, samples=5)
    vol = {"tsdf": torch.zeros((4, 4, 4), device="cuda"), "origin": (-3.0, -3.0, -3.0),
           "spacing": (2.0, 2.0, 2.0)}
    vl = torch.full((4, 4, 4), 1, dtype=torch.int32, device="cuda")
    v = score_voxel_labels_3d(vol, vl, gt["verts"], gt["labels"], 1.8, **kw)
    assert v["sampled"] == ref["n_samples"] and v["vertices"] == scored


def test_score_mesh_3d_sampling_flags_and_unchanged_output_without_them(tmp_path, capsys):
    from scripts import score_mesh_3d
    from tests.test_gpu_surface import parent_mesh_distance
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    from ucsa_neural_rendering_amd.utils.mesh_eval import (mesh_distance, sample_surface,
                                                           score_labels_3d)
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    pred, gt = SyntheticRoom(0).labelled_mesh(0.1), room()["coarse"]
    write_ply(str(tmp_path / "p.ply"), pred["verts"], pred["faces"], labels=pred["labels"])
    write_ply(str(tmp_path / "g.ply"), gt["verts"], gt["faces"], labels=gt["labels"])
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply"),
            "--max_dist", str(MAX_DIST), "--threshold", "0.02"]
    capsys.readouterr()
    # without the flags: the lines of the parent, from strings computed here
    rec = score_mesh_3d.main(args)
    out = capsys.readouterr().out.splitlines()
    s3 = score_labels_3d(pred["verts"], pred["labels"], gt["verts"], gt["labels"], MAX_DIST)
    geo = parent_mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST)
    assert out == ["3d: " + json.dumps(s3), "geometry: " + json.dumps(geo)]
    assert "sampled" not in out[0] and "sampled" not in out[1] and rec == {"3d": s3, "geometry": geo}
    rec = score_mesh_3d.main(args + ["--surface"])
    out = capsys.readouterr().out.splitlines()
    assert "sampled" not in out[0] and "sampled" not in out[1]
    assert rec["geometry"] == mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST,
                                            pred_faces=pred["faces"], gt_faces=gt["faces"])
    # with them: the sample counts of both sides
    dens, seed = 150.0, 4
    n_pred = sample_surface(pred["verts"], pred["faces"], dens, seed)[2]["n_samples"]
    n_gt = SP.sample_mesh_surface(gt["verts"], gt["faces"], dens, seed)["n_samples"]
    flags = ["--sample_density", str(dens), "--sample_seed", str(seed)]
    rec = sampled = score_mesh_3d.main(args + flags)
    out = capsys.readouterr().out.splitlines()
    assert out == ["3d: " + json.dumps(rec["3d"]), "geometry: " + json.dumps(rec["geometry"])]
    assert rec["3d"]["sampled"] == n_gt and rec["geometry"]["sampled"] == [n_pred, n_gt]
    assert "surface" not in rec["3d"] and "surface" not in rec["geometry"]
    assert rec["3d"] == score_labels_3d(pred["verts"], pred["labels"], gt["verts"], gt["labels"],
                                        MAX_DIST, gt_faces=gt["faces"], sample_density=dens, seed=seed)
    rec = score_mesh_3d.main(args + flags + ["--surface"])
    out = capsys.readouterr().out.splitlines()
    geo = mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST, pred_faces=pred["faces"],
                        gt_faces=gt["faces"], sample_density=dens, seed=seed)
    assert rec["geometry"] == geo and geo["sampled"] == [n_pred, n_gt] and geo["recall"] > 0.9
    assert rec["3d"]["sampled"] == n_gt and rec["3d"]["surface"] is True
    assert json.loads(out[1][len("geometry: "):])["sampled"] == [n_pred, n_gt]
    assert json.loads(out[0][len("3d: "):])["sampled"] == n_gt
    # another seed: another set; no faces: refused
    other = score_mesh_3d.main(args + ["--sample_density", str(dens), "--sample_seed", "5"])
    assert other["geometry"] != sampled["geometry"] and other["3d"] != sampled["3d"]
    write_ply(str(tmp_path / "bare.ply"), gt["verts"], labels=gt["labels"])
    with pytest.raises((SystemExit, ValueError)):
        score_mesh_3d.main(["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "bare.ply"),
                            "--sample_density", "10"])
