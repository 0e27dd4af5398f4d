"""GPU: nearest point within a radius (csrc/point_grid.hip: ucsa_point_cell_keys,
ucsa_nearest_point; ops.point_grid, ops.nearest_point) against the brute-force
definition of tests/nearest_numpy.py, byte for byte, on the inputs of
tests/test_nearest_cpu.py: degenerate sizes, exact ties on a shuffled lattice,
duplicated positions, a sparse grid with outliers and non-finite values, every
cell size (0.25 and 0.5 with the lattice on cell walls), sorted and unsorted
queries, twice.  Guard words, unchanged inputs,
argument codes; the 3D scores of utils/mesh_eval.py and the scripts."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import nearest_numpy as NN
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded
from tests.test_nearest_cpu import CELLS, all_cases, same, want

pytestmark = pytest.mark.gpu
F = np.float32


def gpu_nearest(p, q, md, cell=None, sort_queries=True):
    ops = _ops()
    grid = ops.point_grid(_cu(p).view(-1, 3), cell)
    idx, d2 = ops.nearest_point(grid, _cu(q).view(-1, 3), md, sort_queries=sort_queries)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32
    return (idx.cpu().numpy(), d2.cpu().numpy()), grid


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_bytes_equal_the_definition_for_every_cell_size_and_query_order(name):
    p, q, md = all_cases()[name]
    ref = want(name)
    for cell in CELLS:
        for sort_queries in (True, False):
            got, grid = gpu_nearest(p, q, md, cell, sort_queries)
            assert same(got, ref), (name, cell, sort_queries)
        again, _ = gpu_nearest(p, q, md, cell, True)
        assert same(again, ref), (name, cell, "second run")
        # the grid itself: keys, order, offsets and the packed points as restated
        g = NN.point_grid(p, cell)
        assert grid["dims"] == g["dims"] and F(grid["cell"]) == g["cell"]
        assert np.asarray(grid["origin"], F).tobytes() == g["origin"].tobytes()
        for k in ("order", "offsets", "sorted_points"):
            assert grid[k].cpu().numpy().tobytes() == g[k].tobytes(), (name, cell, k)


def raw_call(l, grid, queries, max_dist, out_index, out_dist2, q_order=None, **over):
    """ucsa_nearest_point with the grid's arguments; ``over`` replaces any of them by name"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(sp=grid["sorted_points"], off=grid["offsets"], n=grid["n"],
             origin=(C.c_float * 3)(*grid["origin"]), cell=grid["cell"],
             dims=(C.c_uint32 * 3)(*grid["dims"]), q=queries, order=q_order,
             nq=queries.shape[0], md=max_dist, index=out_index, dist2=out_dist2)
    a.update(over)
    return l.ucsa_nearest_point(p(a["sp"]), p(a["off"]), a["n"], a["origin"], a["cell"], a["dims"],
                                p(a["q"]), p(a["order"]), a["nq"], a["md"], p(a["index"]),
                                p(a["dist2"]), None)


def test_guard_words_and_unchanged_inputs():
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    for name in ("q129", "sparse_0.2"):
        pts, q, md = all_cases()[name]
        ref = want(name)
        P, Q = _cu(pts).view(-1, 3), _cu(q).view(-1, 3)
        grid = ops.point_grid(P, 0.3)
        keep = {k: grid[k].clone() for k in ("sorted_points", "offsets", "order")}
        nq, n = Q.shape[0], P.shape[0]
        keys, check_k = guarded((n,), torch.int32, -5)
        origin, dims = (C.c_float * 3)(*grid["origin"]), (C.c_uint32 * 3)(*grid["dims"])
        assert l.ucsa_point_cell_keys(p(P), n, origin, grid["cell"], dims, 1, p(keys), None) == 0
        index, check_i = guarded((nq,), torch.int32, -5)
        dist2, check_d = guarded((nq,), torch.float32, -5.0)
        perm = _cu(np.random.default_rng(2).permutation(nq).astype(np.int32))
        for order in (None, perm):
            index[:] = -5
            assert raw_call(l, grid, Q, md, index, dist2, order) == 0
            torch.cuda.synchronize()
            for c in (check_k, check_i, check_d):
                c()
            assert same((index.cpu().numpy(), dist2.cpu().numpy()), ref), name
        g = NN.point_grid(pts, 0.3)
        assert keys.cpu().numpy().tobytes() == NN.cell_keys(pts, g["origin"], g["cell"],
                                                            g["dims"]).tobytes()
        qk = torch.empty(nq, dtype=torch.int32, device="cuda")
        assert l.ucsa_point_cell_keys(p(Q), nq, origin, grid["cell"], dims, 0, p(qk), None) == 0
        assert qk.cpu().numpy().tobytes() == NN.cell_keys(q, g["origin"], g["cell"], g["dims"],
                                                          clamp=False).tobytes()
        assert P.cpu().numpy().tobytes() == pts.tobytes() and Q.cpu().numpy().tobytes() == q.tobytes()
        for k, v in keep.items():
            assert torch.equal(grid[k].view(torch.int32), v.view(torch.int32)), k


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    pts, q, md = all_cases()["q65"]
    P, Q = _cu(pts).view(-1, 3), _cu(q).view(-1, 3)
    grid = ops.point_grid(P)
    nq = Q.shape[0]
    index, check_i = guarded((nq,), torch.int32, 99)
    dist2, check_d = guarded((nq,), torch.float32, 99.0)
    f3, u3 = (lambda *v: (C.c_float * 3)(*v)), (lambda *v: (C.c_uint32 * 3)(*v))
    nan, inf = float("nan"), float("inf")
    call = lambda **over: raw_call(l, grid, Q, md, index, dist2, **over)
    for rc, arg in ((call(sp=None), 0), (call(off=None), 1), (call(n=2 ** 31), 2),
                    (call(origin=None), 3), (call(origin=f3(0, nan, 0)), 3),
                    (call(cell=0.0), 4), (call(cell=-1.0), 4), (call(cell=inf), 4),
                    (call(cell=nan), 4), (call(dims=None), 5), (call(dims=u3(4, 0, 4)), 5),
                    (call(dims=u3(257, 256, 256)), 5), (call(dims=u3(65536, 65536, 1)), 5),
                    (call(q=None), 6), (call(nq=2 ** 31), 8), (call(md=0.0), 9),
                    (call(md=-1.0), 9), (call(md=inf), 9), (call(md=nan), 9), (call(md=1e20), 9),
                    (call(index=None), 10), (call(dist2=None), 11)):
        assert rc == -(1000 + arg), (rc, arg)
    keys, check_k = guarded((pts.shape[0],), torch.int32, 99)
    o, d = f3(*grid["origin"]), u3(*grid["dims"])

    def kcall(pp=P, n=pts.shape[0], origin=o, cell=grid["cell"], dims=d, clamp=1, k=keys):
        return l.ucsa_point_cell_keys(p(pp), n, origin, cell, dims, clamp, p(k), None)
    for rc, arg in ((kcall(pp=None), 0), (kcall(n=2 ** 31), 1), (kcall(origin=None), 2),
                    (kcall(origin=f3(inf, 0, 0)), 2), (kcall(cell=0.0), 3), (kcall(cell=nan), 3),
                    (kcall(dims=None), 4), (kcall(dims=u3(0, 1, 1)), 4),
                    (kcall(dims=u3(4097, 4096, 1)), 4), (kcall(clamp=2), 5), (kcall(k=None), 6)):
        assert rc == -(1000 + arg), (rc, arg)
    assert kcall(pp=None, n=0, k=None) == 0                       # legal: launch nothing
    assert call(q=None, nq=0, index=None, dist2=None) == 0
    torch.cuda.synchronize()
    for c in (check_i, check_d, check_k):
        c()
    # an argument error launches nothing: the outputs still hold their fill
    assert (index == 99).all() and (dist2 == 99).all() and (keys == 99).all()
    assert call(sp=None, off=None, n=0) == 0                      # no points: every query -1
    torch.cuda.synchronize()
    assert (index == -1).all() and torch.isinf(dist2).all()
    for bad in (lambda: ops.point_grid(P.cpu()), lambda: ops.point_grid(P[:, :2]),
                lambda: ops.point_grid(P, cell=0.0), lambda: ops.point_grid(P, cell=float("nan")),
                lambda: ops.nearest_point(grid, Q.cpu(), 0.1),
                lambda: ops.nearest_point(grid, Q, 0.0), lambda: ops.nearest_point(grid, Q, inf),
                lambda: ops.nearest_point(grid, Q, 1e20),
                lambda: ops.nearest_point({"n": 1}, Q, 0.1),
                lambda: ops.nearest_point({**grid, "offsets": grid["offsets"][:-1]}, Q, 0.1)):
        with pytest.raises(UcsaError):
            bad()


# ---- the utilities on the analytic room ---------------------------------------
MAX_DIST = 0.1
SHIFT = np.array([0.01, 0.0, 0.0], F)
# what the restatement reaches for the 0.05 mesh's labels at the 0.1 mesh's
# vertices (computed on the CPU from nearest_numpy): every vertex of the coarse
# mesh has a vertex of the fine one within max_dist and all but a few at the
# borders of rectangles, where two classes meet at one position, get their own
# class: mIoU 0.97091, total accuracy 0.97979
FLOOR_MIOU = 0.97


@pytest.fixture(scope="module")
def meshes():
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    room = SyntheticRoom(0)
    gt, pred = room.labelled_mesh(0.1), room.labelled_mesh(0.05)
    idx, d2 = NN.nearest_point_grid(pred["verts"], gt["verts"], MAX_DIST)
    # the grid model is the definition here too: a sample against brute force
    pick = np.random.default_rng(4).choice(gt["verts"].shape[0], 300, replace=False)
    assert same(NN.nearest_point(pred["verts"], gt["verts"][pick], MAX_DIST), (idx[pick], d2[pick]))
    lab = np.where(idx >= 0, pred["labels"].astype(np.int32)[np.maximum(idx, 0)], 0).astype(np.int32)
    return {"gt": gt, "pred": pred, "index": idx, "dist2": d2, "labels": lab}


def confusion_scores(pred, truth, C=40):
    """mIoU, total and class-average accuracy from a confusion matrix built here:
    truth 1..C scored, a prediction outside 1..C a miss"""
    ok = (truth >= 1) & (truth <= C)
    t = truth[ok].astype(np.int64) - 1
    p = pred[ok].astype(np.int64) - 1
    p = np.where((p >= 0) & (p < C), p, (t + 1) % C)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (t, p), 1)
    rows, cols, diag = cm.sum(1).astype(np.float64), cm.sum(0).astype(np.float64), \
        np.diagonal(cm).astype(np.float64)
    pres = rows > 0
    return {"mIoU": float(np.mean((diag / np.maximum(rows + cols - diag, 1))[pres])),
            "total_acc": float(diag.sum() / cm.sum()),
            "mean_acc": float(np.mean((diag / np.maximum(rows, 1))[pres])),
            "vertices": int(ok.sum())}


def test_transfer_and_label_score_equal_the_restatement(meshes):
    from ucsa_neural_rendering_amd.utils.mesh_eval import score_labels_3d, transfer_labels
    gt, pred = meshes["gt"], meshes["pred"]
    got, index, dist2 = transfer_labels(pred["verts"], pred["labels"], gt["verts"], MAX_DIST,
                                        return_match=True)
    assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == meshes["labels"].tobytes()
    assert same((index.cpu().numpy(), dist2.cpu().numpy()), (meshes["index"], meshes["dist2"]))
    s = score_labels_3d(pred["verts"], pred["labels"], gt["verts"], gt["labels"], MAX_DIST)
    ref = confusion_scores(meshes["labels"], np.asarray(gt["labels"]))
    print("3d score of the room:", s, "restated:", ref)
    assert s["vertices"] == ref["vertices"] == gt["verts"].shape[0]
    for k in ("mIoU", "total_acc", "mean_acc"):
        assert abs(s[k] - ref[k]) <= 1e-12, k
    assert s["unmatched"] == float((meshes["index"] < 0).mean()) == 0.0
    assert ref["mIoU"] >= FLOOR_MIOU and s["mIoU"] >= FLOOR_MIOU
    # nothing within reach: every scored vertex unmatched and wrong
    far = score_labels_3d(pred["verts"] + F(100.0), pred["labels"], gt["verts"], gt["labels"], 0.5)
    assert far["unmatched"] == 1.0 and far["total_acc"] == 0.0


def test_mesh_distance_against_float64_numpy(meshes):
    """The ground truth shifted by (0.01, 0, 0).  Against the 0.05 mesh the
    distances agree with a float64 numpy evaluation of the restatement's dist2
    to 1e-9 relative (the float64 summation order over <= 10^5 terms).  The
    F-score of 1 at threshold 0.02 and 0 at 0.005 is asserted for the 0.1 mesh
    against its own shifted copy, where every vertex has its twin exactly 0.01
    away: against the 0.05 mesh it cannot be 1, three of four fine vertices lie
    0.05 or more from any coarse vertex (precision 0.2527, recall 0.9842 at
    0.02, from the restatement).  The reference distances come from the model of
    the traversal; 300 queries of every run are held to the brute force."""
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance
    pred, gt = meshes["pred"]["verts"], meshes["gt"]["verts"]
    gts = (gt + SHIFT).astype(F)
    md = 0.5

    pick = np.random.default_rng(3)

    def one_way(a, b, thr):
        idx, d2 = NN.nearest_point_grid(b, a, md)
        # the reference is the definition, not the model: a sample against brute force
        k = pick.choice(a.shape[0], min(300, a.shape[0]), replace=False)
        assert same(NN.nearest_point(b, a[k], md), (idx[k], d2[k]))
        d = np.where(idx >= 0, np.sqrt(d2.astype(np.float64)), md)
        return float(d.mean()), float(((idx >= 0) & (d <= thr)).mean())
    for name, a in (("fine mesh", pred), ("the mesh itself", gt)):
        for thr in (0.02, 0.005):
            got = mesh_distance(a, gts, thr, md)
            acc, prec = one_way(a, gts, thr)
            comp, rec = one_way(gts, a, thr)
            ref = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp),
                   "precision": prec, "recall": rec,
                   "fscore": 2 * prec * rec / (prec + rec) if prec + rec else 0.0}
            print("mesh_distance,", name, "at", thr, got, "restated:", ref)
            for k, v in ref.items():
                assert abs(got[k] - v) <= 1e-9 * abs(v), (name, thr, k, got[k], v)
            if a is gt:
                assert got["fscore"] == (1.0 if thr == 0.02 else 0.0)
                assert abs(got["accuracy"] - 0.01) < 1e-6 and abs(got["chamfer"] - 0.01) < 1e-6
    # nothing within max_dist: every vertex counts as max_dist
    far = mesh_distance(gt[:500] + F(50.0), gt, 0.02, 0.25)
    assert far["accuracy"] == far["completeness"] == 0.25 and far["fscore"] == 0.0


@pytest.fixture(scope="module")
def voxel_room():
    from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec
    ops = _ops()
    _, poses, intr, depth = room_frames(120, 160)
    dims, origin, h, trunc = room_volume_spec(96)
    vol = ops.tsdf_volume(dims, origin, float(h), with_color=False)
    ops.integrate_tsdf(vol, _cu(depth), _cu(poses), intr, float(trunc))
    # labels on the surface band: a class per octant, 0 off the band
    band = (vol["weight"] >= 1) & (vol["tsdf"].abs() < 0.5)
    i, j, k = torch.meshgrid(*[torch.arange(d, device="cuda") for d in dims], indexing="ij")
    octant = (1 + (i >= dims[0] // 2).int() + 2 * (j >= dims[1] // 2).int()
              + 4 * (k >= dims[2] // 2).int())
    return vol, torch.where(band, octant, torch.zeros_like(octant)).to(torch.int32)


def test_voxel_score_equals_the_mesh_score_of_the_same_centres(meshes, voxel_room):
    from ucsa_neural_rendering_amd.utils.mesh_eval import (score_labels_3d, score_voxel_labels_3d,
                                                            voxel_centres)
    vol, lab = voxel_room
    gt = meshes["gt"]
    centres, cl = voxel_centres(vol, lab)
    assert 1000 < centres.shape[0] < lab.numel() and int(cl.min()) >= 1
    ijk = np.argwhere(lab.cpu().numpy() > 0)
    want_c = (np.asarray(vol["origin"], F)[None, :] + ijk.astype(F) * np.asarray(vol["spacing"], F)[None, :])
    assert centres.cpu().numpy().tobytes() == want_c.astype(F).tobytes()
    a = score_voxel_labels_3d(vol, lab, gt["verts"], gt["labels"], 0.2)
    b = score_labels_3d(centres, cl, gt["verts"], gt["labels"], 0.2)
    assert a == b and a["vertices"] == gt["verts"].shape[0] and 0.0 <= a["unmatched"] < 1.0


# ---- scripts ------------------------------------------------------------------
def lines(capsys, tag):
    out = capsys.readouterr().out.splitlines()
    return [json.loads(ln[len(tag):]) for ln in out if ln.startswith(tag)], out


def test_score_mesh_3d_script_prints_the_numbers_of_the_utilities(meshes, tmp_path, capsys):
    from scripts import score_mesh_3d
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance, score_labels_3d
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    gt, pred = meshes["gt"], meshes["pred"]
    write_ply(str(tmp_path / "p.ply"), pred["verts"], pred["faces"], labels=pred["labels"])
    write_ply(str(tmp_path / "g.ply"), gt["verts"], gt["faces"], labels=gt["labels"])
    write_ply(str(tmp_path / "bare.ply"), gt["verts"], gt["faces"])
    np.savetxt(tmp_path / "T.txt", np.array([[1, 0, 0, 0.01], [0, 1, 0, 0], [0, 0, 1, 0],
                                             [0, 0, 0, 1.0]]))
    capsys.readouterr()
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply")]
    rec = score_mesh_3d.main(args + ["--max_dist", str(MAX_DIST), "--threshold", "0.02"])
    (s3,), out = lines(capsys, "3d: ")
    assert s3 == rec["3d"] == score_labels_3d(pred["verts"], pred["labels"], gt["verts"],
                                              gt["labels"], MAX_DIST)
    (geo,) = [json.loads(ln[len("geometry: "):]) for ln in out if ln.startswith("geometry: ")]
    assert geo == rec["geometry"] == mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST)
    assert s3["mIoU"] >= FLOOR_MIOU and 0.0 < geo["fscore"] < 1.0
    # the shifted ground truth: the numbers of test_mesh_distance_against_float64_numpy
    rec = score_mesh_3d.main(args + ["--max_dist", "0.5", "--threshold", "0.005",
                                     "--gt_transform", str(tmp_path / "T.txt")])
    moved = (gt["verts"].astype(np.float64) + np.array([0.01, 0.0, 0.0])).astype(F)
    assert rec["geometry"] == mesh_distance(pred["verts"], moved, 0.005, 0.5)
    assert rec["3d"] == score_labels_3d(pred["verts"], pred["labels"], moved, gt["labels"], 0.5)
    capsys.readouterr()
    rec = score_mesh_3d.main(["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "bare.ply")])
    got3, out = lines(capsys, "3d: ")
    assert got3 == [] and "3d" not in rec and sum(ln.startswith("geometry: ") for ln in out) == 1


def test_fuse_mesh_labels_gt_mesh_prints_a_3d_line_and_changes_nothing_else(tmp_path, capsys):
    from scripts import fuse_mesh_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=8, H=240, W=320)
    room = SyntheticRoom(0)
    m, g = room.labelled_mesh(0.1), room.labelled_mesh(0.2)
    write_ply(str(tmp_path / "m.ply"), m["verts"], m["faces"])
    write_ply(str(tmp_path / "g.ply"), g["verts"], g["faces"], labels=g["labels"])
    base = ["--scene_root", sroot, "--mesh", str(tmp_path / "m.ply"), "--labels", "label_40"]
    strip = lambda rec: {k: v for k, v in rec.items() if k not in ("fuse_ms_per_view", "out", "3d")}
    capsys.readouterr()
    r0 = fuse_mesh_labels.main(base + ["--out", str(tmp_path / "f0.ply")])
    got0, out0 = lines(capsys, "3d: ")
    r1 = fuse_mesh_labels.main(base + ["--out", str(tmp_path / "f1.ply"), "--gt_mesh",
                                       str(tmp_path / "g.ply"), "--gt_max_dist", "0.15"])
    got1, out1 = lines(capsys, "3d: ")
    assert got0 == [] and "3d" not in r0                             # without the flag: as it was
    assert len(got1) == 1 and got1[0] == r1["3d"] and len(out1) == len(out0) + 1
    rest = [ln for ln in out1 if not ln.startswith("3d: ")]
    assert rest[:-1] == out0[:-1]
    assert strip(json.loads(rest[-1])) == strip(json.loads(out0[-1])) == strip(r0)
    assert open(tmp_path / "f0.ply", "rb").read() == open(tmp_path / "f1.ply", "rb").read()
    s = r1["3d"]
    assert s["vertices"] == g["verts"].shape[0] and 0.0 <= s["unmatched"] < 1.0
    assert 0.0 < s["mIoU"] <= 1.0 and 0.0 < s["total_acc"] <= 1.0


def test_voxel_map_labels_gt_mesh_prints_a_3d_line_and_changes_nothing_else(tmp_path, capsys):
    from scripts import voxel_map_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=8, H=120, W=160)
    g = SyntheticRoom(0).labelled_mesh(0.2)
    write_ply(str(tmp_path / "g.ply"), g["verts"], g["faces"], labels=g["labels"])
    write_ply(str(tmp_path / "bare.ply"), g["verts"], g["faces"])
    base = ["--scene_root", sroot, "--labels", "label_40", "--voxel", "0.08"]
    strip = lambda rec: {k: v for k, v in rec.items()
                         if k not in ("fuse_ms_per_view", "raycast_ms_per_view", "out_dir", "3d")}
    capsys.readouterr()
    r0 = voxel_map_labels.main(base + ["--out_dir", str(tmp_path / "v0")])
    got0, out0 = lines(capsys, "3d: ")
    r1 = voxel_map_labels.main(base + ["--out_dir", str(tmp_path / "v1"), "--gt_mesh",
                                       str(tmp_path / "g.ply"), "--gt_max_dist", "0.15"])
    got1, out1 = lines(capsys, "3d: ")
    assert got0 == [] and "3d" not in r0                             # without the flag: as it was
    assert len(got1) == 1 and got1[0] == r1["3d"] and len(out1) == len(out0) + 1
    rest = [ln for ln in out1 if not ln.startswith("3d: ")]
    assert rest[:-1] == out0[:-1]
    assert strip(json.loads(rest[-1])) == strip(json.loads(out0[-1])) == strip(r0)
    for k in ("map_label", "map_depth"):
        for f in sorted((tmp_path / "v0" / k).iterdir()):
            assert f.read_bytes() == (tmp_path / "v1" / k / f.name).read_bytes()
    s = r1["3d"]
    assert s["vertices"] == g["verts"].shape[0] and 0.0 <= s["unmatched"] < 1.0
    assert 0.0 < s["mIoU"] <= 1.0 and 0.0 < s["total_acc"] <= 1.0
    with pytest.raises(SystemExit):
        voxel_map_labels.main(base + ["--out_dir", str(tmp_path / "v2"), "--gt_mesh",
                                      str(tmp_path / "bare.ply")])
