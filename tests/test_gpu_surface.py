"""GPU: nearest point on a mesh surface within a radius (csrc/triangle_grid.hip:
ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs, ucsa_nearest_triangle;
ops.triangle_grid, ops.nearest_triangle) against the brute-force definition of
tests/surface_numpy.py, byte for byte, on the inputs of
tests/test_surface_cpu.py, at three cell sizes, with sorted and unsorted
queries.  The grid's offsets and records against the model's; guard words,
unchanged inputs, argument codes; the surface variants of utils/mesh_eval.py
and of scripts/score_mesh_3d.py on the analytic room."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import nearest_numpy as NN
from tests import surface_numpy as SN
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded
from tests.test_surface_cpu import NAMES, all_cases, cells_of, room, same, want

pytestmark = pytest.mark.gpu
F = np.float32


def gpu_grid(v, f, cell=None):
    return _ops().triangle_grid(_cu(v).view(-1, 3), _cu(f).view(-1, 3), cell)


def gpu_nearest(grid, q, md, sort_queries=True):
    face, d2, bary = _ops().nearest_triangle(grid, _cu(q).view(-1, 3), md, sort_queries=sort_queries)
    assert face.dtype == torch.int32 and d2.dtype == torch.float32 and bary.dtype == torch.float32
    return face.cpu().numpy(), d2.cpu().numpy(), bary.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_definition_at_three_cell_sizes_and_both_query_orders(name):
    v, f, q, md = all_cases()[name]
    ref = want(name)
    for cell in cells_of(name):
        grid = gpu_grid(v, f, cell)
        for sort_queries in (True, False):
            assert same(gpu_nearest(grid, q, md, sort_queries), ref), (name, cell, sort_queries)
        # the grid itself: shape, offsets and the packed records as restated
        g = SN.triangle_grid(v, f, cell)
        assert grid["dims"] == g["dims"] and F(grid["cell"]) == g["cell"]
        assert np.asarray(grid["origin"], F).tobytes() == g["origin"].tobytes()
        assert grid["n_pairs"] == g["n_pairs"] and grid["n_faces"] == f.shape[0]
        assert grid["records"].shape == (g["n_pairs"], 12)
        for k in ("offsets", "records"):
            assert grid[k].cpu().numpy().tobytes() == g[k].tobytes(), (name, cell, k)


def test_the_two_searches_agree_on_faces_that_are_points():
    """The two instantiations of the one ring walk (pg_walk in csrc/cell_grid.h)
    against each other: over the faces [i, i, i] the face search is the point
    search.  A degenerate face lands in the first corner region, bary (1, 0, 0),
    and its dist2 is the point search's expression on negated differences."""
    ops = _ops()
    rng = np.random.default_rng(17)
    pts = rng.uniform(-1.0, 1.0, (200, 3)).astype(F)
    pts[17] = pts[3]                                             # a tie: the smaller index wins
    pts[40, 1] = np.nan                                          # matches nothing in either search
    faces = np.repeat(np.arange(200, dtype=np.int32)[:, None], 3, axis=1)
    q = np.concatenate([rng.uniform(-1.3, 1.3, (300, 3)).astype(F), pts[:20]])
    P, Fc, Q = _cu(pts).view(-1, 3), _cu(faces).view(-1, 3), _cu(q).view(-1, 3)
    misses = 0
    for md in (0.05, 0.3, 5.0):
        ref_p = NN.nearest_point(pts, q, md)
        ref_t = SN.nearest_triangle(pts, faces, q, md)
        hit = ref_p[0] >= 0
        assert hit.any()
        misses += int((~hit).sum())                              # none at 5.0: every query matches
        for cell in (None, 0.07, 1.5):
            pgrid, tgrid = ops.point_grid(P, cell), ops.triangle_grid(P, Fc, cell)
            for sort_queries in (True, False):
                index, d2p = (t.cpu().numpy() for t in
                              ops.nearest_point(pgrid, Q, md, sort_queries=sort_queries))
                face, d2t, bary = gpu_nearest(tgrid, q, md, sort_queries)
                where = (md, cell, sort_queries)
                assert face.tobytes() == index.tobytes() and d2t.tobytes() == d2p.tobytes(), where
                assert (bary[hit] == np.array([1, 0, 0], F)).all() and (bary[~hit] == 0).all(), where
                assert index.tobytes() == ref_p[0].tobytes() and d2p.tobytes() == ref_p[1].tobytes(), where
                assert same((face, d2t, bary), ref_t), where
    assert misses > 0


def raw_call(l, grid, queries, max_dist, out_face, out_dist2, out_bary, q_order=None, **over):
    """ucsa_nearest_triangle with the grid's arguments; ``over`` replaces any of them by name"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(rec=grid["records"], off=grid["offsets"], n=grid["n_pairs"],
             origin=(C.c_float * 3)(*grid["origin"]), cell=grid["cell"],
             dims=(C.c_uint32 * 3)(*grid["dims"]), q=queries, order=q_order,
             nq=queries.shape[0], md=max_dist, face=out_face, dist2=out_dist2, bary=out_bary)
    a.update(over)
    return l.ucsa_nearest_triangle(p(a["rec"]), p(a["off"]), a["n"], a["origin"], a["cell"],
                                   a["dims"], p(a["q"]), p(a["order"]), a["nq"], a["md"],
                                   p(a["face"]), p(a["dist2"]), p(a["bary"]), None)


def test_guard_words_and_unchanged_inputs():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    for name in ("nonfinite", "spanning"):
        v, f, q, md = all_cases()[name]
        ref = want(name)
        V, Fc, Q = _cu(v).view(-1, 3), _cu(f).view(-1, 3), _cu(q).view(-1, 3)
        cell = cells_of(name)[2]
        grid = _ops().triangle_grid(V, Fc, cell)
        g = SN.triangle_grid(v, f, cell)
        keep = {k: grid[k].clone() for k in ("records", "offsets")}
        nv, nf, nq, P = v.shape[0], f.shape[0], q.shape[0], g["n_pairs"]
        origin, dims = (C.c_float * 3)(*grid["origin"]), (C.c_uint32 * 3)(*grid["dims"])
        counts, check_c = guarded((nf,), torch.int32, -5)
        assert l.ucsa_triangle_cell_counts(p(V), nv, p(Fc), nf, origin, grid["cell"], dims,
                                           p(counts), None) == 0
        keys, check_k = guarded((P,), torch.int32, -5)
        pf, check_p = guarded((P,), torch.int32, -5)
        first = _cu(g["first"])
        assert l.ucsa_triangle_cell_pairs(p(V), nv, p(Fc), nf, origin, grid["cell"], dims,
                                          p(first), P, p(keys), p(pf), None) == 0
        torch.cuda.synchronize()
        for c in (check_c, check_k, check_p):
            c()
        assert counts.cpu().numpy().tobytes() == g["counts"].tobytes()
        assert keys.cpu().numpy().tobytes() == g["keys"].tobytes()
        assert pf.cpu().numpy().tobytes() == g["pair_face"].tobytes()
        # a scan that is not the counts' (shifted up, negative): nothing outside [0, P)
        keys[:] = -5
        pf[:] = -5
        wrong = _cu((g["first"].astype(np.int64) + 7).clip(max=2 ** 31 - 1).astype(np.int32))
        wrong[0] = -3
        assert l.ucsa_triangle_cell_pairs(p(V), nv, p(Fc), nf, origin, grid["cell"], dims,
                                          p(wrong), P, p(keys), p(pf), None) == 0
        torch.cuda.synchronize()
        check_k()
        check_p()
        face, check_f = guarded((nq,), torch.int32, -5)
        dist2, check_d = guarded((nq,), torch.float32, -5.0)
        bary, check_b = guarded((nq, 3), torch.float32, -5.0)
        rng = np.random.default_rng(2)
        perm = _cu(rng.permutation(nq).astype(np.int32))
        for order in (None, perm):
            face[:] = -5
            assert raw_call(l, grid, Q, md, face, dist2, bary, order) == 0
            torch.cuda.synchronize()
            for c in (check_f, check_d, check_b):
                c()
            assert same((face.cpu().numpy(), dist2.cpu().numpy(), bary.cpu().numpy()), ref), name
        # malformed entries of q_order write nothing: their queries keep the fill
        broken = perm.clone()
        broken[:3] = torch.tensor([-1, nq, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
        lost = perm[:3].long()
        face[:] = -5
        dist2[:] = -5.0
        bary[:] = -5.0
        assert raw_call(l, grid, Q, md, face, dist2, bary, broken) == 0
        torch.cuda.synchronize()
        for c in (check_f, check_d, check_b):
            c()
        assert (face[lost] == -5).all() and (dist2[lost] == -5).all() and (bary[lost] == -5).all()
        rest = np.ones(nq, bool)
        rest[lost.cpu().numpy()] = False
        assert face.cpu().numpy()[rest].tobytes() == ref[0][rest].tobytes()
        assert (V.cpu().numpy().tobytes() == v.tobytes() and Fc.cpu().numpy().tobytes() == f.tobytes()
                and Q.cpu().numpy().tobytes() == q.tobytes())
        for k, t in keep.items():
            assert torch.equal(grid[k].view(torch.int32), t.view(torch.int32)), k


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    v, f, q, md = all_cases()["random"]
    V, Fc, Q = _cu(v).view(-1, 3), _cu(f).view(-1, 3), _cu(q[:65]).view(-1, 3)
    grid = ops.triangle_grid(V, Fc)
    nv, nf, nq, P = v.shape[0], f.shape[0], 65, grid["n_pairs"]
    face, check_f = guarded((nq,), torch.int32, 99)
    dist2, check_d = guarded((nq,), torch.float32, 99.0)
    bary, check_b = guarded((nq, 3), torch.float32, 99.0)
    f3, u3 = (lambda *x: (C.c_float * 3)(*x)), (lambda *x: (C.c_uint32 * 3)(*x))
    nan, inf = float("nan"), float("inf")
    call = lambda **over: raw_call(l, grid, Q, md, face, dist2, bary, **over)
    for rc, arg in ((call(rec=None), 0), (call(off=None), 1), (call(n=2 ** 31), 2),
                    (call(origin=None), 3), (call(origin=f3(0, nan, 0)), 3),
                    (call(cell=0.0), 4), (call(cell=-1.0), 4), (call(cell=inf), 4),
                    (call(cell=nan), 4), (call(dims=None), 5), (call(dims=u3(4, 0, 4)), 5),
                    (call(dims=u3(257, 256, 256)), 5), (call(dims=u3(65536, 65536, 1)), 5),
                    (call(q=None), 6), (call(nq=2 ** 31), 8), (call(md=0.0), 9),
                    (call(md=-1.0), 9), (call(md=inf), 9), (call(md=nan), 9), (call(md=1e20), 9),
                    (call(face=None), 10), (call(dist2=None), 11), (call(bary=None), 12)):
        assert rc == -(1000 + arg), (rc, arg)
    counts, check_c = guarded((nf,), torch.int32, 99)
    keys, check_k = guarded((P,), torch.int32, 99)
    pf, check_p = guarded((P,), torch.int32, 99)
    first = torch.zeros(nf, dtype=torch.int32, device="cuda")
    o, d = f3(*grid["origin"]), u3(*grid["dims"])

    def ccall(vv=V, n_v=nv, ff=Fc, n_f=nf, origin=o, cell=grid["cell"], dims=d, out=counts):
        return l.ucsa_triangle_cell_counts(p(vv), n_v, p(ff), n_f, origin, cell, dims, p(out), None)

    def pcall(vv=V, n_v=nv, ff=Fc, n_f=nf, origin=o, cell=grid["cell"], dims=d, fi=first, n=P,
              k=keys, pp=pf):
        return l.ucsa_triangle_cell_pairs(p(vv), n_v, p(ff), n_f, origin, cell, dims, p(fi), n,
                                          p(k), p(pp), None)
    for fn, last in ((ccall, ((dict(out=None), 7),)),
                     (pcall, ((dict(fi=None), 7), (dict(n=2 ** 31), 8), (dict(k=None), 9),
                              (dict(pp=None), 10)))):
        for over, arg in ((dict(vv=None), 0), (dict(n_v=2 ** 31), 1), (dict(ff=None), 2),
                          (dict(n_f=2 ** 31), 3), (dict(origin=None), 4),
                          (dict(origin=f3(inf, 0, 0)), 4), (dict(cell=0.0), 5),
                          (dict(cell=nan), 5), (dict(dims=None), 6), (dict(dims=u3(0, 1, 1)), 6),
                          (dict(dims=u3(4097, 4096, 1)), 6)) + last:
            assert fn(**over) == -(1000 + arg), (fn.__name__, over, arg)
    assert ccall(vv=None, ff=None, n_f=0, out=None) == 0                # legal: launch nothing
    assert pcall(ff=None, n_f=0, fi=None, k=None, pp=None) == 0
    assert pcall(fi=None, n=0, k=None, pp=None) == 0
    assert call(q=None, nq=0, face=None, dist2=None, bary=None) == 0
    torch.cuda.synchronize()
    for c in (check_f, check_d, check_b, check_c, check_k, check_p):
        c()
    # an argument error launches nothing: the outputs still hold their fill
    for t in (face, dist2, bary, counts, keys, pf):
        assert (t == 99).all()
    assert call(rec=None, off=None, n=0) == 0                          # no pairs: no match
    torch.cuda.synchronize()
    for c in (check_f, check_d, check_b):
        c()
    assert (face == -1).all() and torch.isinf(dist2).all() and (bary == 0).all()
    for bad in (lambda: ops.triangle_grid(V.cpu(), Fc), lambda: ops.triangle_grid(V, Fc.cpu()),
                lambda: ops.triangle_grid(V, Fc.long()), lambda: ops.triangle_grid(V, Fc[:, :2]),
                lambda: ops.triangle_grid(V[:, :2], Fc),
                lambda: ops.triangle_grid(V, Fc, cell=0.0),
                lambda: ops.triangle_grid(V, Fc, cell=float("nan")),
                lambda: ops.nearest_triangle(grid, Q.cpu(), 0.1),
                lambda: ops.nearest_triangle(grid, Q, 0.0), lambda: ops.nearest_triangle(grid, Q, inf),
                lambda: ops.nearest_triangle(grid, Q, 1e20),
                lambda: ops.nearest_triangle({"n_pairs": 1}, Q, 0.1),
                lambda: ops.nearest_triangle(ops.point_grid(V), Q, 0.1),
                lambda: ops.nearest_triangle({**grid, "offsets": grid["offsets"][:-1]}, Q, 0.1),
                lambda: ops.nearest_triangle({**grid, "records": grid["records"][:, :8]}, Q, 0.1)):
        with pytest.raises(UcsaError):
            bad()


# ---- the utilities on the analytic room ---------------------------------------
MAX_DIST = 0.5


def model_checked(v, f, q, md, rng):
    """the model's answer, 300 queries of it held to the brute force"""
    out = SN.nearest_triangle_grid(v, f, q, md)
    k = rng.choice(q.shape[0], min(300, q.shape[0]), replace=False)
    assert same(SN.nearest_triangle(v, f, q[k], md), tuple(a[k] for a in out))
    return out


@pytest.fixture(scope="module")
def meshes():
    m = room()
    src, fine = m["coarse"], m["fine"]
    rng = np.random.default_rng(21)
    pick = rng.choice(fine["verts"].shape[0], 20000, replace=False)
    dst, truth = fine["verts"][pick].astype(F), np.asarray(fine["labels"])[pick].astype(np.int32)
    face, d2, bary = model_checked(src["verts"], src["faces"], dst, MAX_DIST, rng)
    corner = np.argmax(bary, axis=1)                                 # the first maximum
    vert = src["faces"][np.maximum(face, 0), corner]
    lab = np.where(face >= 0, np.asarray(src["labels"]).astype(np.int32)[vert], 0).astype(np.int32)
    index = np.where(face >= 0, vert, -1).astype(np.int32)
    return {"src": src, "dst": dst, "truth": truth, "face": face, "dist2": d2, "bary": bary,
            "labels": lab, "index": index}


def test_transfer_labels_with_faces_equals_the_restatement_and_beats_vertices(meshes):
    from ucsa_neural_rendering_amd.utils.mesh_eval import score_labels_3d, transfer_labels
    src, dst, truth = meshes["src"], meshes["dst"], meshes["truth"]
    assert src["faces"].shape[0] == 466
    got, index, dist2, face, bary = transfer_labels(src["verts"], src["labels"], dst, MAX_DIST,
                                                    return_match=True, src_faces=src["faces"])
    assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == meshes["labels"].tobytes()
    assert index.cpu().numpy().tobytes() == meshes["index"].tobytes()
    assert same((face.cpu().numpy(), dist2.cpu().numpy(), bary.cpu().numpy()),
                (meshes["face"], meshes["dist2"], meshes["bary"]))
    only = transfer_labels(src["verts"], src["labels"], dst, MAX_DIST, src_faces=src["faces"])
    assert torch.equal(only, got)
    lab, d2 = got.cpu().numpy(), dist2.cpu().numpy()
    unmatched, exact, agree = (face.cpu().numpy() < 0).mean(), (d2 <= 1e-10).mean(), (lab == truth).mean()
    plain, pidx, _ = transfer_labels(src["verts"], src["labels"], dst, MAX_DIST, return_match=True)
    p_unmatched, p_agree = (pidx.cpu().numpy() < 0).mean(), (plain.cpu().numpy() == truth).mean()
    print("surface: unmatched", unmatched, "dist2 <= 1e-10", exact, "agreement", agree,
          "| vertices: unmatched", p_unmatched, "agreement", p_agree)
    assert unmatched <= 1e-3 and exact >= 0.97 and agree >= 0.97
    assert p_agree <= 0.75 and p_unmatched >= 0.15
    # the score passes the faces through
    s = score_labels_3d(src["verts"], src["labels"], dst, truth, MAX_DIST, pred_faces=src["faces"])
    assert s["vertices"] == 20000 and s["unmatched"] == float(unmatched)
    assert abs(s["total_acc"] - float(agree)) <= 1e-12
    s0 = score_labels_3d(src["verts"], src["labels"], dst, truth, MAX_DIST)
    assert s0["unmatched"] == float(p_unmatched) and abs(s0["total_acc"] - float(p_agree)) <= 1e-12


def parent_mesh_distance(pred, gt, threshold, max_dist):
    """mesh_distance as it was before faces: the same calls and expressions"""
    ops = _ops()
    pred, gt = _cu(pred).view(-1, 3), _cu(gt).view(-1, 3)

    def one_way(a, b):
        index, dist2 = ops.nearest_point(ops.point_grid(b), a, max_dist)
        d = torch.where(index >= 0, dist2.double().sqrt(),
                        torch.full_like(dist2, float(max_dist), dtype=torch.float64))
        return float(d.mean()), float(((index >= 0) & (d <= float(threshold))).double().mean())
    acc, prec = one_way(pred, gt)
    comp, rec = one_way(gt, pred)
    f = 0.0 if prec + rec == 0 else 2.0 * prec * rec / (prec + rec)
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp),
            "precision": prec, "recall": rec, "fscore": f}


@pytest.fixture(scope="module")
def pair():
    """a mesh of the room with faces of its own (step 0.1) against the 466-face one"""
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    return SyntheticRoom(0).labelled_mesh(0.1), room()["coarse"]


def test_mesh_distance_to_the_surface_against_float64_numpy(pair):
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance
    pred, gt = pair
    pv, gv = pred["verts"].astype(F), gt["verts"].astype(F)
    md, thr = MAX_DIST, 0.02
    rng = np.random.default_rng(22)

    def surface(a, bv, bf):
        face, d2, _ = model_checked(bv, bf, a, md, rng)
        d = np.where(face >= 0, np.sqrt(d2.astype(np.float64)), md)
        return float(d.mean()), float(((face >= 0) & (d <= thr)).mean())

    def vertex(a, b):
        idx, d2 = NN.nearest_point_grid(b, a, md)
        d = np.where(idx >= 0, np.sqrt(d2.astype(np.float64)), md)
        return float(d.mean()), float(((idx >= 0) & (d <= thr)).mean())
    to_gt = {True: surface(pv, gv, gt["faces"]), False: vertex(pv, gv)}
    to_pred = {True: surface(gv, pv, pred["faces"]), False: vertex(gv, pv)}
    for gs, ps in ((True, True), (True, False), (False, True)):
        got = mesh_distance(pv, gv, thr, md, pred_faces=pred["faces"] if ps else None,
                            gt_faces=gt["faces"] if gs else None)
        (acc, prec), (comp, rec) = to_gt[gs], to_pred[ps]
        ref = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp),
               "precision": prec, "recall": rec,
               "fscore": 2 * prec * rec / (prec + rec) if prec + rec else 0.0}
        print("mesh_distance, surface", (gs, ps), got, "restated:", ref)
        assert got["surface"] == (gs, ps) and sorted(got) == sorted(list(ref) + ["surface"])
        for k, x in ref.items():
            assert abs(got[k] - x) <= 1e-9 * abs(x), ((gs, ps), k, got[k], x)
    # what the surface is for: the fine vertices lie on the coarse mesh's faces
    assert to_gt[True][0] < 0.01 < 0.1 < to_gt[False][0] and to_gt[True][1] > 0.95 > 0.5 > to_gt[False][1]
    # without faces: what it returned before, to the bit
    plain = mesh_distance(pv, gv, thr, md)
    assert {k: x for k, x in plain.items() if k != "surface"} == parent_mesh_distance(pv, gv, thr, md)
    assert tuple(plain.get("surface", (False, False))) == (False, False)
    # nothing within max_dist: every vertex counts as max_dist
    far = mesh_distance(pv[:500] + F(50.0), gv, thr, 0.25, gt_faces=gt["faces"])
    assert far["accuracy"] == 0.25 and far["precision"] == 0.0


def test_score_mesh_3d_surface_flag_and_unchanged_output_without_it(pair, tmp_path, capsys):
    from scripts import score_mesh_3d
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance, score_labels_3d
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    pred, gt = pair
    write_ply(str(tmp_path / "p.ply"), pred["verts"], pred["faces"], labels=pred["labels"])
    write_ply(str(tmp_path / "g.ply"), gt["verts"], gt["faces"], labels=gt["labels"])
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply"),
            "--max_dist", str(MAX_DIST), "--threshold", "0.02"]
    capsys.readouterr()
    rec = score_mesh_3d.main(args + ["--surface"])
    out = capsys.readouterr().out.splitlines()
    s3 = score_labels_3d(pred["verts"], pred["labels"], gt["verts"], gt["labels"], MAX_DIST,
                         pred_faces=pred["faces"])
    geo = mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST, pred_faces=pred["faces"],
                        gt_faces=gt["faces"])
    assert rec["3d"] == {**s3, "surface": True} and rec["geometry"] == geo
    assert out == ["3d: " + json.dumps({**s3, "surface": True}), "geometry: " + json.dumps(geo)]
    assert json.loads(out[1][len("geometry: "):])["surface"] == [True, True]
    # without the flag: the lines of the parent, from strings computed here
    rec = score_mesh_3d.main(args)
    out = capsys.readouterr().out.splitlines()
    s3 = score_labels_3d(pred["verts"], pred["labels"], gt["verts"], gt["labels"], MAX_DIST)
    geo = parent_mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST)
    assert out == ["3d: " + json.dumps(s3), "geometry: " + json.dumps(geo)]
    assert "surface" not in out[0] and "surface" not in out[1]
    assert rec == {"3d": s3, "geometry": geo}
    # the coarse ground truth: its vertices score the fine mesh's labels either way,
    # the fine mesh's vertices reach the coarse surface only with the flag
    assert rec["geometry"]["precision"] < 0.5 < 0.95 < \
        mesh_distance(pred["verts"], gt["verts"], 0.02, MAX_DIST, gt_faces=gt["faces"])["precision"]
