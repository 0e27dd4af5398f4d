"""GPU: mesh simplification by vertex clustering (csrc/mesh_simplify.hip:
ucsa_vertex_cluster_keys, ucsa_cluster_reduce, ucsa_cluster_faces;
ops.simplify_mesh) against the plain loops of tests/simplify_numpy.py, byte for
byte, on the cases of tests/test_simplify_cpu.py: three cells each, with and
without split_labels, with and without each optional attribute.  Guard words,
unchanged inputs, malformed order / first / vertex_map, argument codes; the
utilities of utils/mesh_fusion.py and the scripts' --simplify on the analytic
room."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import simplify_numpy as SM
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded
from tests.test_simplify_cpu import NAMES, all_cases, want

pytestmark = pytest.mark.gpu
F = np.float32
ARRAYS = ("verts", "count", "normals", "rgb", "labels", "faces", "face_index", "vertex_map")
DTYPES = {"verts": torch.float32, "count": torch.int32, "normals": torch.float32,
          "rgb": torch.uint8, "labels": torch.uint8, "faces": torch.int32,
          "face_index": torch.int32, "vertex_map": torch.int32}


def gpu_simplify(c, cell, split, use=("normals", "rgb", "labels"), **kw):
    opt = {k: _cu(c[k]) for k in use}
    return _ops().simplify_mesh(_cu(c["verts"]).view(-1, 3), _cu(c["faces"]).view(-1, 3), cell,
                                split_labels=split, **opt, **kw)


def assert_same(got, ref, use, tag):
    for k in ARRAYS:
        if k in ("normals", "rgb", "labels") and k not in use:
            assert k not in got, (tag, k)
            continue
        assert got[k].dtype == DTYPES[k] and tuple(got[k].shape) == ref[k].shape, (tag, k)
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), (tag, k)
    assert np.asarray(got["origin"], F).tobytes() == np.asarray(ref["origin"], F).tobytes(), tag
    assert F(got["cell"]) == F(ref["cell"]) and tuple(got["dims"]) == tuple(ref["dims"]), tag
    assert (got["degenerate"], got["duplicate"]) == (ref["degenerate"], ref["duplicate"]), tag


COMBOS = (("normals", "rgb", "labels"), (), ("rgb", "labels"), ("normals", "labels"),
          ("normals", "rgb"))


@pytest.mark.parametrize("name", NAMES)
def test_bytes_equal_the_restatement(name):
    c = all_cases()[name]
    for cell in c["cells"]:
        for split in (False, True):
            for use in COMBOS:
                got = gpu_simplify(c, cell, split, use)
                ref = want(name, cell, split, with_labels="labels" in use)
                assert_same(got, ref, use, (name, cell, split, use))


def test_an_explicit_origin_and_integer_label_dtypes():
    c = all_cases()["random"]
    origin = (-0.37, 0.21, -1.5)
    ref = SM.simplify_mesh(c["verts"], c["faces"], 0.13, normals=c["normals"], rgb=c["rgb"],
                           labels=c["labels"], origin=origin)
    use = ("normals", "rgb", "labels")
    assert_same(gpu_simplify(c, 0.13, False, origin=origin), ref, use, "origin")
    # an origin inside the box: what lies below it is clamped into the first cells
    inside = (0.5, 0.5, 0.5)
    ref2 = SM.simplify_mesh(c["verts"], c["faces"], 0.13, normals=c["normals"], rgb=c["rgb"],
                            labels=c["labels"], origin=inside)
    assert_same(gpu_simplify(c, 0.13, False, origin=inside), ref2, use, "inside")
    for dt in (torch.uint8, torch.int16, torch.int64):
        got = _ops().simplify_mesh(_cu(c["verts"]), _cu(c["faces"]), 0.13, normals=_cu(c["normals"]),
                                   rgb=_cu(c["rgb"]), labels=_cu(c["labels"]).to(dt), origin=origin)
        assert_same(got, ref, use, dt)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_guard_words_unchanged_inputs_and_malformed_lists():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    for name, cell in (("nonfinite", 0.2), ("long", 0.1), ("faces", 0.1)):
        c = all_cases()[name]
        ref = want(name, cell, False)
        n, nf, K = c["verts"].shape[0], c["faces"].shape[0], ref["verts"].shape[0]
        V, Fc, N, R = _cu(c["verts"]), _cu(c["faces"]), _cu(c["normals"]), _cu(c["rgb"])
        L = _cu(c["labels"].astype(np.uint8))
        origin, dims = (C.c_float * 3)(*ref["origin"]), (C.c_uint32 * 3)(*ref["dims"])
        keys, ck = guarded((n,), torch.int64, -5)
        assert l.ucsa_vertex_cluster_keys(_p(V), n, origin, ref["cell"], dims, _p(L), _p(keys),
                                          None) == 0
        torch.cuda.synchronize()
        ck()
        assert keys.cpu().numpy().tobytes() == ref["keys"].tobytes()
        order, first = _cu(ref["order"]), _cu(ref["first"])
        ov, c1 = guarded((K, 3), torch.float32, -5.0)
        on, c2 = guarded((K, 3), torch.float32, -5.0)
        oc, c3 = guarded((K, 3), torch.uint8, 9)
        ol, c4 = guarded((K,), torch.uint8, 9)
        ok, c5 = guarded((K,), torch.int32, -5)
        checks = (c1, c2, c3, c4, c5)

        def reduce_(order=order, first=first):
            rc = l.ucsa_cluster_reduce(_p(V), _p(N), _p(R), _p(L), n, _p(order), _p(first), K,
                                       _p(ov), _p(on), _p(oc), _p(ol), _p(ok), None)
            torch.cuda.synchronize()
            for ch in checks:
                ch()
            return rc
        assert reduce_() == 0
        for t, k in ((ov, "verts"), (on, "normals"), (oc, "rgb"), (ol, "labels"), (ok, "count")):
            assert t.cpu().numpy().tobytes() == ref[k].tobytes(), (name, k)
        # malformed entries: -1, n, 2^31-1 in order; negative, too large and decreasing offsets
        bad_o = order.clone()
        bad_o[:3] = torch.tensor([-1, n, 2 ** 31 - 1], dtype=torch.int32, device="cuda")
        assert reduce_(order=bad_o) == 0
        bad_f = first.clone()
        bad_f[0] = -1
        bad_f[K // 2] = 2 ** 31 - 1
        bad_f[K - 1] = n
        bad_f[K] = 0
        assert reduce_(first=bad_f) == 0
        assert reduce_(order=bad_o, first=bad_f) == 0
        # faces
        vm = _cu(ref["vertex_map"])
        tri, c6 = guarded((nf, 3), torch.int32, -5)
        keep, c7 = guarded((nf,), torch.uint8, 9)
        assert l.ucsa_cluster_faces(_p(Fc), nf, _p(vm), n, _p(tri), _p(keep), None) == 0
        torch.cuda.synchronize()
        c6()
        c7()
        assert tri.cpu().numpy().tobytes() == ref["tri"].tobytes()
        assert keep.cpu().numpy().tobytes() == ref["keep"].tobytes()
        bad_v = vm.clone()
        bad_v[:4] = torch.tensor([-1, n, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device="cuda")
        assert l.ucsa_cluster_faces(_p(Fc), nf, _p(bad_v), n, _p(tri), _p(keep), None) == 0
        torch.cuda.synchronize()
        c6()
        c7()
        want_t, want_k = SM.cluster_faces(c["faces"], bad_v.cpu().numpy())
        assert tri.cpu().numpy().tobytes() == want_t.tobytes()
        assert keep.cpu().numpy().tobytes() == want_k.tobytes()
        # the wrapper leaves its inputs alone as well
        _ops().simplify_mesh(V, Fc, cell, normals=N, rgb=R, labels=L, split_labels=True)
        for t, a in ((V, c["verts"]), (Fc, c["faces"]), (N, c["normals"]), (R, c["rgb"]),
                     (L, c["labels"].astype(np.uint8)), (order, ref["order"]), (first, ref["first"]),
                     (vm, ref["vertex_map"])):
            assert t.cpu().numpy().tobytes() == a.tobytes(), name


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    c = all_cases()["random"]
    ref = want("random", 0.13, False)
    n, nf, K = c["verts"].shape[0], c["faces"].shape[0], ref["verts"].shape[0]
    V, Fc, N, R = _cu(c["verts"]), _cu(c["faces"]), _cu(c["normals"]), _cu(c["rgb"])
    L = _cu(c["labels"].astype(np.uint8))
    f3, u3 = (lambda *x: (C.c_float * 3)(*x)), (lambda *x: (C.c_uint32 * 3)(*x))
    nan, inf = float("nan"), float("inf")
    keys, ck = guarded((n,), torch.int64, 99)
    outs = [guarded((K, 3), torch.float32, 99.0), guarded((K, 3), torch.float32, 99.0),
            guarded((K, 3), torch.uint8, 99), guarded((K,), torch.uint8, 99),
            guarded((K,), torch.int32, 99)]
    ov, on, oc, ol, ok = (t for t, _ in outs)
    tri, ct = guarded((nf, 3), torch.int32, 99)
    keep, cp = guarded((nf,), torch.uint8, 99)
    order, first, vm = _cu(ref["order"]), _cu(ref["first"]), _cu(ref["vertex_map"])

    def kcall(v=V, n_=n, origin=f3(*ref["origin"]), cell=ref["cell"], dims=u3(*ref["dims"]), lab=L,
              out=keys):
        return l.ucsa_vertex_cluster_keys(_p(v), n_, origin, cell, dims, _p(lab), _p(out), None)

    def rcall(v=V, nr=N, rg=R, lab=L, n_=n, o=order, f=first, k=K, a=ov, b=on, cc=oc, d=ol, e=ok):
        return l.ucsa_cluster_reduce(_p(v), _p(nr), _p(rg), _p(lab), n_, _p(o), _p(f), k, _p(a),
                                     _p(b), _p(cc), _p(d), _p(e), None)

    def fcall(f=Fc, nf_=nf, m=vm, nv=n, t=tri, k=keep):
        return l.ucsa_cluster_faces(_p(f), nf_, _p(m), nv, _p(t), _p(k), None)
    for rc, arg in ((kcall(v=None), 0), (kcall(n_=2 ** 31), 1), (kcall(origin=None), 2),
                    (kcall(origin=f3(0, nan, 0)), 2), (kcall(origin=f3(inf, 0, 0)), 2),
                    (kcall(cell=0.0), 3), (kcall(cell=-1.0), 3), (kcall(cell=inf), 3),
                    (kcall(cell=nan), 3), (kcall(cell=3e38, dims=u3(4, 4, 4)), 3),
                    (kcall(dims=None), 4), (kcall(dims=u3(4, 0, 4)), 4),
                    (kcall(dims=u3(2 ** 18 + 1, 1, 1)), 4), (kcall(out=None), 6),
                    (rcall(v=None), 0), (rcall(n_=2 ** 31), 4), (rcall(o=None), 5),
                    (rcall(f=None), 6), (rcall(k=n + 1), 7), (rcall(a=None), 8), (rcall(b=None), 9),
                    (rcall(cc=None), 10), (rcall(d=None), 11), (rcall(e=None), 12),
                    (fcall(f=None), 0), (fcall(nf_=2 ** 31), 1), (fcall(m=None), 2),
                    (fcall(nv=2 ** 31), 3), (fcall(t=None), 4), (fcall(k=None), 5)):
        assert rc == -(1000 + arg), (rc, arg)
    # legal: nothing to do, nothing launched
    assert kcall(v=None, n_=0, out=None) == 0
    assert rcall(v=None, o=None, f=None, k=0, a=None, b=None, cc=None, d=None, e=None) == 0
    assert fcall(f=None, nf_=0, t=None, k=None) == 0
    torch.cuda.synchronize()
    for t in (keys, ov, on, oc, ol, ok, tri, keep):
        assert (t == 99).all()                                # an argument error launches nothing
    # 2^18 cells along an axis is the limit and is accepted; absent attributes need no output
    assert kcall(dims=u3(2 ** 18, 2 ** 18, 2 ** 18), cell=1e-3) == 0
    assert rcall(nr=None, rg=None, lab=None, b=None, cc=None, d=None) == 0
    assert fcall(m=None, nv=0) == 0                           # no vertices: every face dropped
    torch.cuda.synchronize()
    for ch in [ck, ct, cp] + [x for _, x in outs]:
        ch()
    assert (on == 99).all() and (oc == 99).all() and (ol == 99).all()
    assert (tri == -1).all() and (keep == 0).all()
    lab64 = _cu(c["labels"].astype(np.int64))
    for bad in (lambda: ops.simplify_mesh(V.cpu(), Fc, 0.1), lambda: ops.simplify_mesh(V, Fc.cpu(), 0.1),
                lambda: ops.simplify_mesh(V, Fc.long(), 0.1),
                lambda: ops.simplify_mesh(V, Fc[:, :2], 0.1),
                lambda: ops.simplify_mesh(V[:, :2], Fc, 0.1),
                lambda: ops.simplify_mesh(V, Fc, 0.0), lambda: ops.simplify_mesh(V, Fc, -1.0),
                lambda: ops.simplify_mesh(V, Fc, nan), lambda: ops.simplify_mesh(V, Fc, inf),
                lambda: ops.simplify_mesh(V, Fc, 1e-6),          # more than 2^18 cells
                lambda: ops.simplify_mesh(V, Fc, 0.1, labels=lab64 - 1),
                lambda: ops.simplify_mesh(V, Fc, 0.1, labels=lab64 + 251),
                lambda: ops.simplify_mesh(V, Fc, 0.1, labels=lab64.float()),
                lambda: ops.simplify_mesh(V, Fc, 0.1, labels=lab64.cpu()),
                lambda: ops.simplify_mesh(V, Fc, 0.1, labels=lab64[:-1]),
                lambda: ops.simplify_mesh(V, Fc, 0.1, normals=N.cpu()),
                lambda: ops.simplify_mesh(V, Fc, 0.1, normals=N[:-1]),
                lambda: ops.simplify_mesh(V, Fc, 0.1, rgb=R.cpu()),
                lambda: ops.simplify_mesh(V, Fc, 0.1, rgb=R.float()),
                lambda: ops.simplify_mesh(V, Fc, 0.1, origin=(0.0, nan, 0.0)),
                lambda: ops.simplify_mesh(V, Fc, 0.1, origin=(0.0, 0.0))):
        with pytest.raises(UcsaError):
            bad()
    with pytest.raises(UcsaError, match="raise cell"):
        ops.simplify_mesh(V, Fc, 1e-6)


# ---- the utilities and the scripts on the analytic room ------------------------
def test_mesh_fusion_simplify_and_pool_on_the_room():
    from ucsa_neural_rendering_amd.utils.mesh_fusion import pool_label_table, simplify_mesh
    c = all_cases()["room"]
    fcls = np.arange(c["faces"].shape[0], dtype=np.int64) % 7
    mesh = {"verts": c["verts"], "faces": c["faces"], "normals": c["normals"], "rgb": c["rgb"],
            "labels": c["labels"], "face_classes": fcls, "note": "kept"}
    for split in (False, True):
        ref = want("room", 0.25, split)
        got, st = simplify_mesh(mesh, 0.25, split_labels=split)
        for k in ("verts", "faces", "normals", "rgb", "vertex_map", "face_index"):
            assert got[k].dtype == ref[k].dtype and got[k].tobytes() == ref[k].tobytes(), (split, k)
        assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], ref["labels"])
        assert np.array_equal(got["face_classes"], fcls[ref["face_index"]]) and got["note"] == "kept"
        assert st == {"vertices": [c["verts"].shape[0], ref["verts"].shape[0]],
                      "faces": [c["faces"].shape[0], ref["faces"].shape[0]],
                      "degenerate": ref["degenerate"], "duplicate": ref["duplicate"],
                      "largest_cluster": int(ref["count"].max())}
        print("simplify_mesh on the room, split", split, st)
    assert mesh["verts"] is c["verts"] and "vertex_map" not in mesh
    # float colours in [0,1] (load_mesh's) go through write_ply's rounding and come back as floats
    ref = want("room", 0.25, False)
    bare = {"verts": c["verts"], "faces": c["faces"], "labels": None,
            "rgb": c["rgb"].astype(F) / F(255.0)}
    got, _ = simplify_mesh(bare, 0.25)
    no_labels = want("room", 0.25, False, with_labels=False)
    assert got["verts"].tobytes() == no_labels["verts"].tobytes() and got["labels"] is None
    assert got["rgb"].dtype == F and "normals" not in got
    assert np.array_equal(np.round(got["rgb"].astype(np.float64) * 255.0).astype(np.uint8),
                          no_labels["rgb"])
    # a table fused on the fine mesh, resolved on the coarse one
    rng = np.random.default_rng(43)
    pick = rng.choice(c["verts"].shape[0], 4000, replace=False)
    vm = np.full(c["verts"].shape[0], -1, np.int32)
    vm[pick] = ref["vertex_map"][pick]
    table = np.zeros((c["verts"].shape[0], 9), np.int64)
    table[pick] = rng.integers(-2 ** 63, 2 ** 63, (4000, 9), dtype=np.int64)
    K = ref["verts"].shape[0]
    T = _cu(table)
    pooled = pool_label_table(T, vm, K)
    assert pooled.dtype == torch.int64 and pooled.is_cuda
    assert pooled.cpu().numpy().tobytes() == SM.pool_label_table(table[pick], vm[pick], K).tobytes()
    assert torch.equal(pool_label_table(T, _cu(vm), K), pooled) and T.cpu().numpy().tobytes() == table.tobytes()
    with pytest.raises(ValueError):
        pool_label_table(T, vm, int(vm.max()))               # a row mapped past the output


def _rows(ply, renormalise=False):
    """the vertex records of a PLY as a sorted table, and position -> index"""
    v = ply["vertex"].copy()
    if renormalise:
        # a cluster of one: s = 0 + n, then the contract's n / len, in float32
        s = [F(0) + v[k] for k in ("nx", "ny", "nz")]
        ln = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        assert ln.dtype == F
        with np.errstate(all="ignore"):
            for k, x in zip(("nx", "ny", "nz"), s):
                v[k] = np.where(ln > 0, x / ln, F(0))
    where = {ply["verts"][i].tobytes(): i for i in range(ply["verts"].shape[0])}
    return np.sort(v, order=list(v.dtype.names)), where


def _same_up_to_vertex_order(a, b):
    """PLY ``b`` is PLY ``a`` with its vertices renumbered and its faces rotated.
    Positions, colours and labels keep their bits; a normal has gone once more
    through the normalisation that the contract applies to every cluster's sum,
    which is restated here exactly (no tolerance)."""
    ra, _ = _rows(a, renormalise=True)
    rb, where = _rows(b)
    assert len(where) == a["verts"].shape[0], "positions must be distinct"
    assert ra.tobytes() == rb.tobytes()
    m = np.asarray([where[a["verts"][i].tobytes()] for i in range(a["verts"].shape[0])])[a["faces"]]
    r = np.argmin(m, axis=1)
    rot = np.stack([m[np.arange(len(m)), (r + k) % 3] for k in range(3)], 1)
    assert np.array_equal(rot, b["faces"])


def _cell_below_the_vertex_spacing(verts):
    """the largest of a few cells at which no two vertices share a cell"""
    for cell in (1e-3, 3e-4, 1e-4, 5e-5):
        o, c, dims = SM.grid_of(verts, cell)
        if np.unique(SM.cluster_keys(verts, o, c, dims)).size == verts.shape[0]:
            return cell
    raise AssertionError("two vertices of the mesh lie within 5e-5 of each other")


def test_scripts_simplify_flag_and_unchanged_bytes_without_it(tmp_path, capsys):
    """the scene and sizes of tests/test_gpu_components.py's script test"""
    from scripts import fuse_mesh_labels, fuse_tsdf_mesh
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply
    Hs, Ws, n = 240, 320, 8
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=Hs, W=Ws)
    h = 6.1 / 63
    box = ["--voxel", repr(h), "--aabb", "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05"]

    def stats_line():
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("simplify: ")]
        return [json.loads(ln[len("simplify: "):]) for ln in lines]

    tsdf = ["--scene_root", sroot] + box
    capsys.readouterr()
    r = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "t.ply")])
    assert stats_line() == [] and "simplify" not in r
    fine = read_ply(str(tmp_path / "t.ply"))
    rs = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "ts.ply"), "--simplify", "0.3",
                                     "--min_component", "50"])
    (st,) = stats_line()
    ply = read_ply(str(tmp_path / "ts.ply"))
    assert st == rs["simplify"] and st["vertices"][1] == rs["vertices"] == ply["verts"].shape[0]
    assert st["faces"][1] == rs["faces"] == ply["faces"].shape[0] and "normals" in ply and "rgb" in ply
    assert 0 < st["vertices"][1] < st["vertices"][0] <= r["vertices"] and st["largest_cluster"] > 1
    assert ply["faces"].max() < rs["vertices"]
    # a cell below the vertex spacing: the same mesh, vertices in cell order
    tiny = _cell_below_the_vertex_spacing(fine["verts"])
    rt = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "tt.ply"), "--simplify", repr(tiny)])
    (st,) = stats_line()
    assert st == {"vertices": [r["vertices"]] * 2, "faces": [r["faces"]] * 2, "degenerate": 0,
                  "duplicate": 0, "largest_cluster": 1} and rt["vertices"] == r["vertices"]
    _same_up_to_vertex_order(fine, read_ply(str(tmp_path / "tt.ply")))
    # labels fused onto the TSDF mesh
    fus = ["--scene_root", sroot, "--mesh", str(tmp_path / "t.ply"), "--labels", "label_40"]
    f0 = fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "f.ply")])
    assert stats_line() == [] and "simplify" not in f0
    fs = fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "fs.ply"), "--simplify", "0.3",
                                      "--simplify_split_labels"])
    (st,) = stats_line()
    ply = read_ply(str(tmp_path / "fs.ply"))
    assert st == fs["simplify"] and st["vertices"] == [r["vertices"], ply["verts"].shape[0]]
    assert fs["vertices"] == ply["verts"].shape[0] and fs["faces"] == ply["faces"].shape[0] == st["faces"][1]
    assert "labels" in ply and "normals" in ply and "rgb" in ply and fs["observed"] > 0
    ft = fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "ft.ply"), "--simplify", repr(tiny)])
    (st,) = stats_line()
    assert st["vertices"] == [r["vertices"]] * 2 and st["largest_cluster"] == 1
    assert ft["observed"] == f0["observed"]
    _same_up_to_vertex_order(read_ply(str(tmp_path / "f.ply")), read_ply(str(tmp_path / "ft.ply")))
