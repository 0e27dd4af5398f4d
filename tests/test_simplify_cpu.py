"""CPU-only: properties of the vertex-clustering restatement
(tests/simplify_numpy.py) on the cases that tests/test_gpu_simplify.py holds the
kernels to, byte for byte.  Nothing here touches a GPU.

The numbers of the README (the analytic room's 0.05 mesh at cell 0.25) are
printed by ``test_room_figures_for_the_readme``; they are recorded, not
asserted.  Only the derived distance bound is asserted."""
import math

import numpy as np
import pytest

from tests import simplify_numpy as SM
from tests import surface_numpy as SN
from tests.test_surface_cpu import room

F = np.float32
U = 2.0 ** -24          # the unit roundoff of float32


def _attrs(rng, n, n_labels=6):
    nrm = rng.standard_normal((n, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F)
    return {"normals": nrm.astype(F), "rgb": rng.integers(0, 256, (n, 3)).astype(np.uint8),
            "labels": rng.integers(0, n_labels, n).astype(np.int32)}


def random_case():
    rng = np.random.default_rng(31)
    v = rng.random((3000, 3)).astype(F)
    f = rng.integers(0, 3000, (6000, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **_attrs(rng, 3000), "cells": [0.05, 0.13, 0.37]}


def walls_case():
    """coordinates exactly at origin + k * cell, the box's maximum corner among them"""
    rng = np.random.default_rng(32)
    k = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), -1)
    k = k.reshape(-1, 3)
    v = (k.astype(F) * F(0.25) + np.array([-1.0, 2.0, 0.5], F)).astype(F)
    inner = (k < np.array([8, 6, 4])).all(1)                 # the box stays the lattice's
    v = np.concatenate([v, v[inner][::3] + F(0.0625)]).astype(F)
    n = v.shape[0]
    f = rng.integers(0, n, (700, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **_attrs(rng, n), "cells": [0.25, 0.5, 0.125]}


def nonfinite_case():
    c = random_case()
    v = c["verts"][:1200].copy()
    rng = np.random.default_rng(33)
    bad = rng.choice(1200, 60, replace=False)
    v[bad[:20], rng.integers(0, 3, 20)] = np.nan
    v[bad[20:40], rng.integers(0, 3, 20)] = np.inf
    v[bad[40:], rng.integers(0, 3, 20)] = -np.inf
    f = rng.integers(0, 1200, (2500, 3)).astype(np.int32)
    f[:60, 1] = bad                                          # faces that touch them
    return {"verts": v, "faces": f, **{k: c[k][:1200] for k in ("normals", "rgb", "labels")},
            "cells": [0.07, 0.2, 0.6]}


def flat_case():
    c = random_case()
    v = c["verts"][:1500].copy()
    v[:, 2] = F(0.375)
    f = np.random.default_rng(34).integers(0, 1500, (3000, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **{k: c[k][:1500] for k in ("normals", "rgb", "labels")},
            "cells": [0.04, 0.11, 0.3]}


def onecell_case():
    c = random_case()
    return {**{k: c[k][:800] for k in ("verts", "normals", "rgb", "labels")},
            "faces": c["faces"][:900] % 800, "cells": [1.0, 2.5, 40.0]}


def long_case():
    """one cluster of 5 000 members next to 300 singletons"""
    rng = np.random.default_rng(35)
    blob = (rng.random((5000, 3)) * 0.09).astype(F)
    blob[0] = 0.0
    k = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(3), indexing="ij"), -1)
    single = (k.reshape(-1, 3).astype(F) * F(0.5) + np.array([1.0, 0.0, 0.0], F)).astype(F)
    v = np.concatenate([blob, single]).astype(F)
    perm = rng.permutation(v.shape[0])
    v = v[perm]
    f = rng.integers(0, v.shape[0], (2000, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **_attrs(rng, v.shape[0]), "cells": [0.1, 0.15, 0.2]}


def blocks_case(n):
    """exactly n clusters at cell 1: the last lane of a block and the first of the next"""
    rng = np.random.default_rng(36 + n)
    x = np.arange(n, dtype=F)
    v = np.zeros((2 * n, 3), F)
    v[:n, 0], v[n:, 0] = x + F(0.25), x + F(0.5)
    v[:, 1:] = (rng.random((2 * n, 2)) * 0.9).astype(F)
    v[0] = (0.0, 0.0, 0.0)
    f = rng.integers(0, 2 * n, (3 * n, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **_attrs(rng, 2 * n), "cells": [1.0, 0.5, 2.0]}


def ties_case():
    """equal label counts, all labels 0, label 255"""
    groups = [[3, 3, 2, 2, 0], [0, 0, 0], [255, 255, 1], [0, 0, 0, 7], [5, 4], [9, 9, 9, 1, 1, 1],
              [255], [200, 100, 200, 100, 50]]
    rng = np.random.default_rng(37)
    v, lab = [], []
    for g, labels in enumerate(groups):
        for l in labels:
            v.append([g + 0.1 + 0.8 * rng.random(), 0.8 * rng.random(), 0.8 * rng.random()])
            lab.append(l)
    v = np.asarray(v, F)
    v[0] = (0.0, 0.0, 0.0)
    n = v.shape[0]
    a = _attrs(rng, n)
    a["labels"] = np.asarray(lab, np.int32)
    f = rng.integers(0, n, (60, 3)).astype(np.int32)
    return {"verts": v, "faces": f, **a, "cells": [1.0, 2.0, 0.5]}


def faces_case():
    """repeated faces, reversed copies, rotated copies, corner indices -1 and >= V,
    faces degenerate on input"""
    rng = np.random.default_rng(38)
    n = 300
    v = rng.random((n, 3)).astype(F)
    base = rng.integers(0, n, (400, 3)).astype(np.int32)
    f = np.concatenate([base, base[:100], base[100:200, ::-1], base[200:300][:, [1, 2, 0]],
                        base[300:350][:, [2, 0, 1]], base[50:80]]).astype(np.int32)
    f = f[rng.permutation(f.shape[0])]
    f[5] = (-1, 3, 4)
    f[6] = (3, n, 4)
    f[7] = (3, 4, 2 ** 31 - 1)
    f[8] = (10, 10, 11)
    f[9] = (12, 13, 12)
    f[10] = (-2 ** 31, 1, 2)
    return {"verts": v, "faces": f, **_attrs(rng, n), "cells": [0.02, 0.1, 0.3]}


def room_case():
    fine = room()["fine"]
    n = fine["verts"].shape[0]
    a = _attrs(np.random.default_rng(39), n)
    a["labels"] = np.asarray(fine["labels"]).astype(np.int32)
    return {"verts": fine["verts"].astype(F), "faces": fine["faces"].astype(np.int32), **a,
            "cells": [0.25]}


_CASES = {}


def all_cases():
    """name -> dict: verts, faces, normals, rgb, labels and the cells to run at (shared:
    do not write)"""
    if not _CASES:
        r = random_case()
        _CASES["random"] = r
        _CASES["shifted"] = {**r, "verts": (r["verts"] + F(1000)).astype(F)}
        _CASES["walls"] = walls_case()
        _CASES["nonfinite"] = nonfinite_case()
        _CASES["flat"] = flat_case()
        _CASES["onecell"] = onecell_case()
        _CASES["long"] = long_case()
        for n in (255, 256, 257, 513):
            _CASES[f"blocks{n}"] = blocks_case(n)
        _CASES["ties"] = ties_case()
        _CASES["faces"] = faces_case()
        _CASES["v0"] = {**{k: r[k][:0] for k in ("verts", "normals", "rgb", "labels")},
                        "faces": r["faces"][:4], "cells": r["cells"]}
        _CASES["f0"] = {**r, "faces": r["faces"][:0]}
        _CASES["room"] = room_case()
        for c in _CASES.values():
            for a in c.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return _CASES


NAMES = ["random", "shifted", "walls", "nonfinite", "flat", "onecell", "long", "blocks255",
         "blocks256", "blocks257", "blocks513", "ties", "faces", "v0", "f0", "room"]

_WANT = {}


def want(name, cell, split, with_labels=True):
    """the restatement's answer with normals and colours, with or without labels,
    computed once and shared (read-only)"""
    key = (name, cell, bool(split), bool(with_labels))
    if key not in _WANT:
        c = all_cases()[name]
        out = SM.simplify_mesh(c["verts"], c["faces"], cell, normals=c["normals"], rgb=c["rgb"],
                               labels=c["labels"] if with_labels else None, split_labels=split)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WANT[key] = out
    return _WANT[key]


def allowance(cell, largest, biggest_cluster):
    """How far, per axis, a member may lie from its cluster's computed vertex, from
    the float32 expressions; M = ``largest`` bounds |coordinate| and |origin|.
    * membership: t = fl(fl(p - o) / cell) has floor k, and both roundings are
      relative, so (p - o) lies within |p - o| * (2u + u^2) <= 5uM of [k cell,
      (k+1) cell]; a vertex clamped into the last cell lies within the same of
      its top wall.  Two members differ by at most D = cell + 10uM per axis, and
      so does a member from the exact mean.
    * the computed mean: d_i = fl(x_i - x0) is off by u D each; the sequential
      sum of n such terms by at most (n-1) u * n D (1+u); divided by n that is
      (n + 1) u D (1 + few u), the division adds u D, the last add u (M + D)."""
    D = cell + 10 * U * largest
    return D * (1.0 + (biggest_cluster + 4) * U * 1.01) + U * largest


@pytest.mark.parametrize("name", NAMES)
def test_properties_of_the_restatement(name):
    c = all_cases()[name]
    v, f = c["verts"], c["faces"]
    fin = np.isfinite(v).all(1)
    for cell in c["cells"]:
        for split in (False, True):
            out = want(name, cell, split)
            K = out["verts"].shape[0]
            vm = out["vertex_map"]
            # count: sums to the finite vertices and agrees with vertex_map
            assert out["count"].sum() == fin.sum() and (out["count"] >= 1).all()
            assert ((vm >= 0) == fin).all() and vm.max(initial=-1) < K
            assert np.array_equal(np.bincount(vm[fin], minlength=K), out["count"])
            # the distance bound
            if fin.any():
                big = float(np.abs(v[fin]).max())
                big = max(big, float(np.abs(np.asarray(out["origin"])).max()))
                e = allowance(float(out["cell"]), big, int(out["count"].max()))
                d = v[fin].astype(np.float64) - out["verts"][vm[fin]].astype(np.float64)
                worst = float(np.sqrt((d * d).sum(1)).max())
                bound = float(out["cell"]) * math.sqrt(3) + math.sqrt(3) * (e - float(out["cell"]))
                assert worst <= bound, (name, cell, split, worst, bound)
            # faces: no degenerate one, no repeated triple, no index >= K
            fo = out["faces"]
            assert fo.dtype == np.int32 and out["face_index"].dtype == np.int32
            if fo.size:
                assert fo.min() >= 0 and fo.max() < K
                assert (fo[:, 0] != fo[:, 1]).all() and (fo[:, 1] != fo[:, 2]).all() \
                    and (fo[:, 0] != fo[:, 2]).all()
                assert (fo[:, 0] < fo[:, 1]).all() and (fo[:, 0] < fo[:, 2]).all()
                assert len({tuple(t) for t in fo.tolist()}) == fo.shape[0]
            assert (np.diff(out["face_index"]) > 0).all()
            assert fo.shape[0] + out["degenerate"] + out["duplicate"] == f.shape[0]
            # split: a cluster holds one label, and it is the output's
            if split and K:
                assert np.array_equal(out["labels"][vm[fin]], c["labels"][fin])
            if "normals" in out and K:
                ln = np.linalg.norm(out["normals"].astype(np.float64), axis=1)
                assert (np.abs(ln - 1.0) < 1e-6)[ln > 0].all()


def test_the_cases_hold_what_they_are_for():
    assert sorted(all_cases()) == sorted(NAMES)
    for n in (255, 256, 257, 513):
        assert want(f"blocks{n}", 1.0, False)["verts"].shape[0] == n
    lg = want("long", 0.1, False)
    assert sorted(lg["count"].tolist())[-2:] == [1, 5000] and lg["verts"].shape[0] == 301
    for cell in all_cases()["onecell"]["cells"]:
        one = want("onecell", cell, False)
        # a cell no smaller than the bounding box: one vertex and no face
        assert one["verts"].shape[0] == 1 and one["faces"].shape[0] == 0 and one["dims"] == (1, 1, 1)
    t = want("ties", 1.0, False)
    assert t["labels"].tolist() == [2, 0, 255, 7, 4, 1, 255, 100]
    assert want("ties", 1.0, True)["verts"].shape[0] == 3 + 1 + 2 + 2 + 2 + 2 + 1 + 3
    w = want("walls", 0.25, False)
    assert w["dims"] == (9, 7, 5) and w["verts"].shape[0] == 9 * 7 * 5
    nf = want("nonfinite", 0.2, False)
    assert (nf["vertex_map"] < 0).sum() == 60 and nf["degenerate"] >= 60
    assert want("flat", 0.11, False)["dims"][2] == 1
    fc = want("faces", 0.02, False)
    assert fc["duplicate"] >= 260 and fc["degenerate"] >= 6     # 280 copies, less the few overwritten
    assert want("v0", 0.05, False)["verts"].shape == (0, 3)
    assert want("v0", 0.05, False)["faces"].shape == (0, 3) and want("v0", 0.05, False)["degenerate"] == 4
    assert want("f0", 0.05, False)["faces"].shape == (0, 3)


def welded_sheet():
    rng = np.random.default_rng(40)
    nx, ny = 12, 9
    x, y = np.meshgrid(np.arange(nx, dtype=F), np.arange(ny, dtype=F), indexing="ij")
    v = np.stack([x, y, rng.random((nx, ny)).astype(F)], -1).reshape(-1, 3).astype(F)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    q = np.stack([a, b, c, d], -1).reshape(-1, 4)
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int32)
    perm = rng.permutation(v.shape[0])                       # so that renumbering is real
    inv = np.argsort(perm)
    return v[perm], inv[f].astype(np.int32)


def test_a_cell_below_the_vertex_spacing_returns_the_mesh_itself():
    v, f = welded_sheet()
    rng = np.random.default_rng(41)
    a = _attrs(rng, v.shape[0])
    out = SM.simplify_mesh(v, f, 0.3, **a)
    vm = out["vertex_map"]
    assert out["verts"].shape == v.shape and (out["count"] == 1).all()
    assert sorted(vm.tolist()) == list(range(v.shape[0]))
    # the vertex set is the input's, bit for bit (and its colours and labels)
    assert out["verts"][vm].tobytes() == v.tobytes()
    assert out["rgb"][vm].tobytes() == a["rgb"].tobytes()
    assert np.array_equal(out["labels"][vm], a["labels"])
    assert np.abs(out["normals"][vm] - a["normals"]).max() < 1e-6
    # the faces are the input's up to renumbering and rotation
    assert out["degenerate"] == 0 and out["duplicate"] == 0
    assert np.array_equal(out["face_index"], np.arange(f.shape[0]))
    m = vm[f]
    r = np.argmin(m, axis=1)
    rot = np.stack([m[np.arange(len(m)), (r + k) % 3] for k in range(3)], 1)
    assert np.array_equal(out["faces"], rot)


def test_pool_label_table_equals_a_numpy_loop():
    rng = np.random.default_rng(42)
    V, C, K = 500, 7, 40
    t = rng.integers(0, 2 ** 63, (V, C + 1), dtype=np.int64) * 2 + rng.integers(0, 2, (V, C + 1))
    vm = rng.integers(-1, K, V).astype(np.int32)
    got = SM.pool_label_table(t, vm, K)
    ref = [[0] * (C + 1) for _ in range(K)]
    for i in range(V):
        if vm[i] >= 0:
            for c in range(C + 1):
                ref[vm[i]][c] = (ref[vm[i]][c] + int(t[i, c].view(np.uint64))) % 2 ** 64
    assert got.dtype == np.int64 and got.view(np.uint64).tolist() == ref
    assert (vm < 0).any() and t.view(np.uint64).max() > 2 ** 63


def test_room_figures_for_the_readme():
    """recorded, not asserted: counts, distance to the analytic surface, label agreement.
    As measured: 92 915 -> 3 610 vertices, 181 350 -> 7 224 faces (3 863 vertices with
    split_labels); distance to the 466-face mesh mean 0.0045, 95th percentile 0.013 (split:
    0.0040 and 8e-8); 99.4 % of the labels equal to the carried one (split: 96.1 %)."""
    m = room()
    src = m["coarse"]
    cell = 0.25
    plain, split = want("room", cell, False), want("room", cell, True)
    print("room 0.05 ->", cell, ": vertices", all_cases()["room"]["verts"].shape[0], "->",
          plain["verts"].shape[0], "faces", all_cases()["room"]["faces"].shape[0], "->",
          plain["faces"].shape[0], "| split_labels: vertices", split["verts"].shape[0], "faces",
          split["faces"].shape[0])
    for name, out in (("plain", plain), ("split", split)):
        face, d2, bary = SN.nearest_triangle_grid(src["verts"].astype(F), src["faces"], out["verts"],
                                                  1.0)
        d = np.sqrt(d2[face >= 0].astype(np.float64))
        corner = np.argmax(bary, axis=1)
        carried = np.asarray(src["labels"]).astype(np.int64)[src["faces"][np.maximum(face, 0), corner]]
        agree = (out["labels"].astype(np.int64) == carried)[face >= 0].mean()
        print(name, ": distance to the 466-face mesh mean", d.mean(), "p95", np.percentile(d, 95),
              "max", d.max(), "| labels equal to the carried one", agree)
    assert plain["verts"].shape[0] > 0
