"""GPU: the scores of many rigid hypotheses against a TSDF volume
(csrc/tsdf_score.hip: ucsa_tsdf_score_transforms; ops.register.tsdf_scores)
against the restatement of tests/global_register_numpy.py as int64 words; the
search of utils.registration.global_register_points_tsdf against the
restatement's search, bit for bit; global_register_meshes and the script's
--register_global on a small mesh pair; argument errors and guard words.  The
inputs and the gates of the search are those of
tests/test_global_register_cpu.py (figures: docs/DESIGN_NOTEBOOK.md, GR)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import global_register_numpy as GR
from tests.test_global_register_cpu import (COARSE_TRUNC, N_POINTS, POINT_SEED, SEARCH_GATE_ROT,
                                            SEARCH_GATE_TRANS, cell_points, coarse_room,
                                            constant_volume, moved_source, unknown_move)
from tests.test_gpu_tsdf_fusion import _ops
from tests.test_gpu_tsdf_register import _cu, gpu_volume
from tests.test_register_cpu import pose_error
from tests.test_tsdf_register_cpu import (PILLAR, ROOM_HALF, ROOM_RADIUS, ROOM_TRUNC, ROOM_VOXEL,
                                          ROOM_Z, room_points, room_volume)
from ucsa_neural_rendering_amd.utils import registration as REG

pytestmark = pytest.mark.gpu
F = np.float32
TILE = 16                                        # UCSA_TSDF_SCORE_TILE

LATTICES = {"cell": ((2, 2, 2), (0.5, 0.4, 0.6), (-0.2, 0.1, 0.3)),
            "small": ((9, 10, 11), (0.1, 0.07, 0.13), (-0.35, 0.4, -0.6)),
            "odd": ((33, 20, 17), (0.05, 0.06, 0.055), (-0.9, 0.4, -0.4))}
SIZES = [0, 1, 255, 256, 257]                    # each with every K of COUNTS (K_MANY transforms)
COUNTS = [0, 1, 2, TILE - 1, TILE, TILE + 1, 1000]
N_MANY, K_FEW = 4099, TILE + 1                   # and 4 099 points with the K up to TILE + 1


def random_volume(name):
    """a smooth field clamped to [-1, 1] with noise, so that inliers, free space and
    the far side all occur; weights 0..3 with a random observed mask"""
    dims, spacing, origin = LATTICES[name]
    g = np.random.default_rng(len(name) + 7)
    i, j, k = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")
    f = 1.3 * np.sin(0.55 * i + 0.3) * np.cos(0.45 * j - 0.2) + 0.8 * np.sin(0.5 * k + 0.1 * i)
    tsdf = np.clip(f + g.normal(0, 0.05, dims), -1.0, 1.0).astype(F)
    weight = g.integers(1, 4, dims).astype(F)
    if name != "cell":
        weight[g.random(dims) < 0.03] = 0.0
    return {"tsdf": tsdf, "weight": weight, "rgb": None, "origin": np.asarray(origin, F),
            "spacing": np.asarray(spacing, F)}


def box_of(vol):
    dims = np.array(vol["tsdf"].shape)
    top = (vol["origin"] + (dims - 1).astype(F) * vol["spacing"]).astype(F)
    return vol["origin"], top


def world_points(vol, n, seed):
    """``n`` float32 points: inside the lattice's box and up to a third of it outside;
    the first rows (n permitting) are the six face centres, their neighbours one ulp
    outside, the eight corners, and NaN / inf rows"""
    g = np.random.default_rng(seed)
    o, top = box_of(vol)
    ext = (top - o).astype(np.float64)
    p = (o + g.uniform(-0.33, 1.33, (n, 3)) * ext).astype(F)
    inside = g.random(n) < 0.7
    p[inside] = (o + g.uniform(0, 1, (int(inside.sum()), 3)) * ext).astype(F)
    mid = ((o + top) * F(0.5)).astype(F)
    special = []
    for a in range(3):
        for side, away in ((o, -np.inf), (top, np.inf)):
            on = mid.copy()
            on[a] = side[a]
            off = on.copy()
            off[a] = np.nextafter(side[a], F(away))
            special += [on, off]
    special += [np.array([(o, top)[i][0], (o, top)[j][1], (o, top)[k][2]], F)
                for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    special += [np.array(r, F) for r in ([np.nan, mid[1], mid[2]], [mid[0], np.inf, mid[2]],
                                         [mid[0], mid[1], -np.inf], [np.nan] * 3)]
    m = min(n, len(special))
    p[:m] = np.array(special[:m], F)
    return p


def some_transforms(vol, K, seed):
    """[K,3,4] float32: the identity first, then turns of up to 40 deg about the box's
    centre with shifts of up to a fifth of it, and rows with NaN, inf and huge entries"""
    g = np.random.default_rng(seed)
    o, top = box_of(vol)
    c = 0.5 * (o.astype(np.float64) + top)
    T = np.empty((K, 3, 4), np.float64)
    for k in range(K):
        axis = g.normal(size=3)
        M = REG.compose(np.eye(4), np.concatenate(
            [np.radians(g.uniform(0, 40)) * axis / np.linalg.norm(axis), np.zeros(3)]))
        T[k, :, :3] = M[:3, :3]
        T[k, :, 3] = c - M[:3, :3] @ c + g.uniform(-0.2, 0.2, 3) * (top - o)
    if K:
        T[0] = np.eye(4)[:3]
    for k, (r, col, v) in zip((3, 7, 11, 13), ((0, 0, np.nan), (1, 3, np.inf), (2, 2, -np.inf),
                                                (0, 3, 3e38))):
        if k < K:
            T[k, r, col] = v
    return T.astype(F)


def pair_table(vol, P, T, min_weight, max_tsdf):
    """the restatement per (transform, point) -> int64 [K,N,4]: inlier, free, e, e^2"""
    K, n = T.shape[0], P.shape[0]
    q = GR._move_many(P, GR.transform_rows(T))
    inlier, free, e = (x.reshape(K, n) for x in GR.point_scores(vol, q, min_weight, max_tsdf))
    return np.stack([inlier.astype(np.int64), free.astype(np.int64), e, e * e], -1)


def words(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("name", sorted(LATTICES))
def test_scores_equal_the_restatement_as_int64_words(name):
    ops = _ops()
    vol = random_volume(name)
    gvol = gpu_volume(vol)
    checked, seen = 0, np.zeros(3, np.int64)
    for (n_all, k_all, sizes, counts) in ((max(SIZES), max(COUNTS), SIZES, COUNTS),
                                          (N_MANY, K_FEW, [N_MANY], COUNTS[:-1])):
        P = world_points(vol, n_all, 300 + n_all)
        T = some_transforms(vol, k_all, 5 + k_all)
        gP, gT = _cu(P), _cu(T)
        perm = np.random.default_rng(n_all).permutation(n_all)
        gPp = _cu(P[perm])
        for min_weight in (1.0, 2.0):
            for max_tsdf in (0.75, 0.5):
                table = pair_table(vol, P, T, min_weight, max_tsdf)
                assert GR.tsdf_scores(vol, P, T, min_weight, max_tsdf).tobytes() == \
                    table.sum(1).tobytes()
                seen += [table[..., 0].sum(), table[..., 1].sum(),
                         (table[..., 0] + table[..., 1] == 0).sum()]
                for n in sizes:
                    for K in counts:
                        where = (name, n, K, min_weight, max_tsdf)
                        want = np.ascontiguousarray(table[:K, :n].sum(1))
                        got = ops.register.tsdf_scores(gvol, gP[:n], gT[:K], min_weight, max_tsdf)
                        assert got.dtype == torch.int64 and tuple(got.shape) == (K, 4)
                        assert got.device == gP.device and words(got) == want.tobytes(), where
                        again = ops.register.tsdf_scores(gvol, gP[:n], gT[:K], min_weight,
                                                         max_tsdf)
                        assert words(again) == want.tobytes(), where
                        checked += 1
                # a shuffled point order: the same bytes, not close ones
                for K in (1, TILE + 1):
                    got = ops.register.tsdf_scores(gvol, gPp, gT[:K], min_weight, max_tsdf)
                    assert words(got) == np.ascontiguousarray(table[:K].sum(1)).tobytes()
                # [K,4,4] transforms: the first three rows are taken
                T4 = torch.zeros((K_FEW, 4, 4), device="cuda")
                T4[:, :3], T4[:, 3] = gT[:K_FEW], 7.0
                got = ops.register.tsdf_scores(gvol, gP, T4, min_weight, max_tsdf)
                assert words(got) == np.ascontiguousarray(table[:K_FEW].sum(1)).tobytes()
        assert words(gP) == P.tobytes() and words(gT) == T.tobytes()      # inputs untouched
    assert checked == 4 * (len(SIZES) * len(COUNTS) + len(COUNTS) - 1)
    assert (seen > 1000).all(), seen                     # inliers, free space and neither
    assert words(gvol["tsdf"]) == vol["tsdf"].tobytes()
    assert words(gvol["weight"]) == vol["weight"].tobytes()


def test_a_call_that_needs_two_launches_equals_the_restatement():
    """more than 65 535 tiles of transforms: the entry point splits the grid"""
    ops = _ops()
    vol = random_volume("small")
    K = 65535 * TILE + TILE + 1
    g = np.random.default_rng(12)
    base = some_transforms(vol, 64, 3)
    T = base[g.integers(0, 64, K)]
    T[:, :, 3] += g.uniform(-0.05, 0.05, (K, 3)).astype(F)
    P = world_points(vol, 30, 1)[[0, 2, 12]]             # two face centres and a corner
    want = GR.tsdf_scores(vol, P, T)
    got = ops.register.tsdf_scores(gpu_volume(vol), _cu(P), _cu(T))
    assert words(got) == want.tobytes() and want[:, 0].sum() > K // 2
    assert want[-(TILE + 1):].any()


def test_the_largest_point_set_with_the_largest_transform_set_equals_the_restatement():
    """N = 4 099 with K = 1 000 (the cross of test_scores... stops at K = TILE + 1 for it):
    17 work-groups of points add to each of 63 tiles' rows"""
    ops = _ops()
    vol = random_volume("odd")
    P, T = world_points(vol, N_MANY, 77), some_transforms(vol, max(COUNTS), 78)
    want = GR.tsdf_scores(vol, P, T)
    got = ops.register.tsdf_scores(gpu_volume(vol), _cu(P), _cu(T))
    assert words(got) == want.tobytes() and (want[:, 0] > 0).sum() > 900


def test_the_gate_and_the_rounding_ties_equal_the_restatement():
    ops = _ops()
    p = cell_points()
    gp = _cu(p)
    eye = torch.eye(4, device="cuda")[None, :3].contiguous()
    at, above = F(0.75), np.nextafter(F(0.75), F(1))
    ties = [F((2 * m + 1) / 2.0 ** 21) for m in (0, 1, 2, 3, 1001, 1002, 393214, 393215)]
    for value in [at, above, -at, -above, F(1.0), F(-1.0), F(np.nan), F(np.inf), F(0.0),
                  F(2.0 ** -140)] + ties + [-t for t in ties]:
        vol = constant_volume(value)
        want = GR.tsdf_scores(vol, p, np.eye(4)[None, :3], 1.0, 0.75)
        got = ops.register.tsdf_scores(gpu_volume(vol), gp, eye, 1.0, 0.75)
        assert words(got) == want.tobytes(), value
    n, e = len(p), int(at * 2.0 ** 20)
    got = ops.register.tsdf_scores(gpu_volume(constant_volume(at)), gp, eye)
    assert got.cpu().tolist() == [[n, 0, n * e, n * e * e]]
    got = ops.register.tsdf_scores(gpu_volume(constant_volume(above)), gp, eye)
    assert got.cpu().tolist() == [[0, n, 0, 0]]
    # one unobserved corner
    vol = constant_volume(F(0.25))
    vol["weight"][4, 5, 6] = 0.0
    q = cell_points(200, 9)
    want = GR.tsdf_scores(vol, q, np.eye(4)[None, :3])
    assert 0 < want[0, 0] < 200
    assert words(ops.register.tsdf_scores(gpu_volume(vol), _cu(q), eye)) == want.tobytes()


# ---- arguments -------------------------------------------------------------------------
def test_argument_errors_come_before_the_library(monkeypatch):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    vol = gpu_volume(random_volume("small"))
    pts = _cu(world_points(random_volume("small"), 10, 0))
    T = _cu(some_transforms(random_volume("small"), 5, 1))

    def boom(*a, **k):
        raise AssertionError("the op reached lib()")
    monkeypatch.setattr(ops.register, "lib", boom)
    call = ops.register.tsdf_scores
    bad = [lambda: call(vol, pts.cpu(), T),
           lambda: call({**vol, "tsdf": vol["tsdf"].cpu()}, pts, T),
           lambda: call({**vol, "weight": vol["weight"][:-1]}, pts, T),
           lambda: call({**vol, "spacing": (0.1, 0.0, 0.1)}, pts, T),
           lambda: call({**vol, "origin": (0.0, float("nan"), 0.0)}, pts, T),
           lambda: call(vol, pts.double(), T),
           lambda: call(vol, pts[:, :2], T),
           lambda: call(vol, pts, T.cpu()),
           lambda: call(vol, pts, T.double()),
           lambda: call(vol, pts, T.cpu().numpy()),
           lambda: call(vol, pts, T[0]),
           lambda: call(vol, pts, T.reshape(5, 12)),
           lambda: call(vol, pts, T[:, :2]),
           lambda: call(vol, pts, T, min_weight=0.0),
           lambda: call(vol, pts, T, min_weight=float("nan")),
           lambda: call(vol, pts, T, max_tsdf=0.0),
           lambda: call(vol, pts, T, max_tsdf=1.0),
           lambda: call(vol, pts, T, max_tsdf=float("nan")),
           lambda: call({**vol, "tsdf": vol["tsdf"][:1].contiguous(),
                         "weight": vol["weight"][:1].contiguous()}, pts, T)]
    for k, c in enumerate(bad):
        with pytest.raises(_lib.UcsaError):
            c()


def test_every_limit_returns_its_index_before_any_launch_and_the_guard_words_survive():
    from ucsa_neural_rendering_amd import _lib
    host = random_volume("small")
    vol = gpu_volume(host)
    P = world_points(host, 300, 2)
    T = some_transforms(host, 40, 2)
    pts, gT = _cu(P), _cu(T)
    l = _lib.lib()
    GUARD, K = 0x5A5A5A5A5A5A5A5A, 40
    buf = torch.full((8 + 4 * K + 8,), GUARD, dtype=torch.int64, device="cuda")
    scores = buf[8:8 + 4 * K]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f3 = lambda v: (C.c_float * 3)(*v)

    def raw(**over):
        a = dict(tsdf=vol["tsdf"], weight=vol["weight"], dims=(9, 10, 11), origin=f3(vol["origin"]),
                 spacing=f3(vol["spacing"]), pts=pts, n=300, T=gT, K=K, mw=1.0, mt=0.75,
                 scores=scores)
        a.update(over)
        return l.ucsa_tsdf_score_transforms(p(a["tsdf"]), p(a["weight"]), *a["dims"], a["origin"],
                                            a["spacing"], p(a["pts"]), a["n"], p(a["T"]), a["K"],
                                            a["mw"], a["mt"], p(a["scores"]), None)
    assert raw(tsdf=None) == -1000 and raw(weight=None) == -1001
    assert raw(dims=(1, 10, 11)) == -1002 and raw(dims=(2048, 2048, 2048)) == -1002
    assert raw(dims=(9, 1, 11)) == -1003 and raw(dims=(9, 10, 1)) == -1004
    assert raw(origin=f3((0.0, float("inf"), 0.0))) == -1005 and raw(origin=None) == -1005
    assert raw(spacing=f3((0.1, -0.1, 0.1))) == -1006 and raw(spacing=None) == -1006
    assert raw(pts=None) == -1007 and raw(n=(1 << 23) + 1) == -1008
    assert raw(T=None) == -1009 and raw(K=1 << 31) == -1010
    assert raw(mw=0.0) == -1011 and raw(mw=float("nan")) == -1011
    assert raw(mt=0.0) == -1012 and raw(mt=1.0) == -1012 and raw(mt=float("nan")) == -1012
    assert raw(scores=None) == -1013
    torch.cuda.synchronize()
    assert (buf == GUARD).all()                          # nothing was written
    assert raw(K=0, T=None, scores=None) == 0            # nothing to do
    torch.cuda.synchronize()
    assert (buf == GUARD).all()
    assert raw(n=0, pts=None) == 0                       # zeroed, nothing that reads points
    torch.cuda.synchronize()
    assert not scores.any() and (buf[:8] == GUARD).all() and (buf[-8:] == GUARD).all()
    buf.fill_(GUARD)
    assert raw() == 0
    torch.cuda.synchronize()
    assert words(scores) == GR.tsdf_scores(host, P, T).tobytes()
    assert (buf[:8] == GUARD).all() and (buf[-8:] == GUARD).all()
    assert words(pts) == P.tobytes() and words(gT) == T.tobytes()


# ---- the search ---------------------------------------------------------------------------
def test_the_search_on_the_room_equals_the_restatements_search_bit_for_bit():
    pts = room_points(N_POINTS, POINT_SEED)
    fine, coarse = room_volume(), coarse_room()
    gfine, gcoarse = gpu_volume(fine), gpu_volume(coarse)
    assert REG.surface_centroid(gcoarse, COARSE_TRUNC).tobytes() == \
        REG.surface_centroid(coarse, COARSE_TRUNC).tobytes()
    for seed in (3, 4):                                  # turns of 158.7 and 121.0 deg
        src, M = moved_source(pts, seed)
        ref = GR.global_register_points_tsdf(src, fine, ROOM_TRUNC, coarse, COARSE_TRUNC)
        got = REG.global_register_points_tsdf(_cu(src), gfine, ROOM_TRUNC, gcoarse, COARSE_TRUNC)
        assert got["n_hypotheses"] == ref["n_hypotheses"] == 4096
        assert len(got["candidates"]) == len(ref["candidates"]) == 16
        for a, b in zip(got["candidates"], ref["candidates"]):
            assert a["index"] == b["index"] and a["score"] == b["score"]
            assert a["coarse_score"] == b["coarse_score"]
            assert a["transform"].tobytes() == b["transform"].tobytes()
        assert got["transform"].tobytes() == ref["transform"].tobytes()
        assert got["score"] == ref["score"] and got["ambiguous"] == ref["ambiguous"] is False
        assert sorted(got) == sorted(ref) == sorted(
            ["ambiguous", "candidates", "converged", "history", "iterations", "matched",
             "n_hypotheses", "n_points", "rank", "rmse", "score", "transform"])
        rot, trans = pose_error(got["transform"], M)
        print(f"seed {seed}, a turn of {unknown_move(seed)[1]:.1f} deg: rot {rot:.4e} rad, trans "
              f"{trans:.4e}, score {got['score']}")
        assert rot <= SEARCH_GATE_ROT and trans <= SEARCH_GATE_TRANS


# ---- meshes -----------------------------------------------------------------------------------
def rectangle(corner, eu, ev, nu, nv, normal):
    """a rectangle as 2 nu nv triangles whose (B-A)x(C-A) points along ``normal``"""
    corner, eu, ev = (np.asarray(x, np.float64) for x in (corner, eu, ev))
    verts = np.array([corner + eu * i / nu + ev * j / nv for i in range(nu + 1)
                      for j in range(nv + 1)])
    idx = lambda i, j: i * (nv + 1) + j
    faces = []
    for i in range(nu):
        for j in range(nv):
            faces += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)),
                      (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    faces = np.array(faces, np.int64)
    if np.dot(np.cross(eu, ev), normal) < 0:
        faces = faces[:, ::-1]
    return verts, faces


def room_mesh():
    """the analytic room with its pillar as 232 triangles, counter-clockwise seen from
    free space: the walls face inward, the pillar outward"""
    lo = np.array([-ROOM_HALF, -ROOM_HALF, ROOM_Z[0]])
    hi = np.array([ROOM_HALF, ROOM_HALF, ROOM_Z[1]])
    parts = []
    for (l, h, sign, n, skip) in ((lo, hi, 1.0, 4, None), (PILLAR[0], PILLAR[1], -1.0, 2, (2, 0))):
        for a in range(3):
            u, v = [b for b in range(3) if b != a]
            for s, side in enumerate((l, h)):
                if skip == (a, s):
                    continue                             # the pillar stands on the floor
                corner = l.copy()
                corner[a] = side[a]
                eu, ev, nrm = np.zeros(3), np.zeros(3), np.zeros(3)
                eu[u], ev[v] = h[u] - l[u], h[v] - l[v]
                nrm[a] = sign * (1.0 if s == 0 else -1.0)
                parts.append(rectangle(corner, eu, ev, n, n, nrm))
    verts, faces, base = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + base)
        base += len(v)
    return {"verts": np.concatenate(verts).astype(F), "faces": np.concatenate(faces).astype(np.int32)}


# The gate of the mesh pair comes from the number format, not from a run: a volume made
# from a mesh holds the exact distance to its planar faces (rounded once), so the fixed
# point of the loop is limited by float32 alone.  A source vertex is rounded once after
# the inverse move and a sample once more, the moved point once after the forward move:
# three half-ulps of a coordinate below 4 (ulp 2^-21 = 4.8e-7), 7e-7 per point and
# coordinate in the worst case.  A pose fitted to 500 such points cannot be farther off
# than its worst point; 32 ulps (1.5e-5 units, and the angle that subtends at the room's
# radius) leave a factor of 20 for the trilinear arithmetic and the solve.
# Measured on the MI355X, seed 3 (a turn of 158.7 deg), 507 samples, voxel 0.05:
# rot 2.3128e-08 rad, trans 8.0056e-08, all 507 points inliers.
MESH_GATE_TRANS = 32 * 2.0 ** -21
MESH_GATE_ROT = MESH_GATE_TRANS / ROOM_RADIUS
assert MESH_GATE_TRANS < 1e-3 * 0.5 * ROOM_VOXEL


def moved_mesh(seed):
    mesh = room_mesh()
    M, angle = unknown_move(seed)
    inv = np.linalg.inv(M)
    moved = (mesh["verts"].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(F)
    return {"verts": moved, "faces": mesh["faces"]}, mesh, M, angle


def test_a_mesh_pair_turned_by_more_than_ninety_degrees_ends_within_the_recorded_gate():
    src, dst, M, angle = moved_mesh(3)
    assert angle > 90.0 and len(dst["faces"]) == 232
    out = REG.global_register_meshes(src, dst, ROOM_VOXEL, samples=512)
    rot, trans = pose_error(out["transform"], M)
    far = [c for c in out["candidates"][1:] if REG.transform_distance(
        c["transform"], out["transform"], src["verts"].astype(np.float64).mean(0))[0] > 0.1]
    print(f"mesh pair, a turn of {angle:.1f} deg: rot {rot:.4e} rad, trans {trans:.4e}, score "
          f"{out['score']} of {out['n_points']} points, ambiguous {out['ambiguous']}, the best "
          f"candidate elsewhere {far[0]['score'] if far else None}")
    assert out["n_hypotheses"] == 4096 and out["rank"] == 6
    assert out["score"][1] == 0                      # a mesh's volume is observed in its band only
    assert rot <= MESH_GATE_ROT and trans <= MESH_GATE_TRANS


def test_script_registers_globally_before_it_scores_and_is_unchanged_without_the_flag(tmp_path,
                                                                                       capsys):
    from scripts import score_mesh_3d
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    src, dst, M, _ = moved_mesh(3)
    write_ply(str(tmp_path / "p.ply"), src["verts"], src["faces"])
    write_ply(str(tmp_path / "g.ply"), dst["verts"], dst["faces"])
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply"), "--surface"]
    capsys.readouterr()
    plain = score_mesh_3d.main(args)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and lines[0] == "geometry: " + json.dumps(plain["geometry"])
    assert sorted(plain) == ["geometry"]
    rec = score_mesh_3d.main(args + ["--register_global", "--register_global_voxel",
                                     str(ROOM_VOXEL), "--register", "--register_max_dist", "0.1"])
    lines = capsys.readouterr().out.strip().splitlines()
    assert [l.split(":")[0] for l in lines] == ["register_global", "register", "geometry"]
    line = json.loads(lines[0][len("register_global: "):])
    assert line == rec["register_global"] and line["n_hypotheses"] == 4096
    assert sorted(line) == ["ambiguous", "n_hypotheses", "points", "rank", "rmse", "score",
                            "transform", "voxel"]
    assert isinstance(line["ambiguous"], bool) and len(line["score"]) == 4
    rot, trans = pose_error(np.array(line["transform"]), M)
    assert rot <= MESH_GATE_ROT and trans <= MESH_GATE_TRANS
    # the refinement started from the search's result: it moves by less than half a voxel
    step = np.array(rec["register"]["transform"])
    assert pose_error(step, np.eye(4))[1] <= 0.5 * ROOM_VOXEL
    assert rec["geometry"]["chamfer"] < 0.1 * plain["geometry"]["chamfer"]
    with pytest.raises(SystemExit):
        score_mesh_3d.main(args + ["--register_global", "--register_global_keep", "0"])
