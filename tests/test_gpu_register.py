"""GPU: the fused ICP step (csrc/mesh_register.hip: ucsa_icp_sums;
ops.register.icp_sums) against the restatement of tests/register_numpy.py, byte
for byte: the 29 sums as int64 words, the matches, at three cell sizes, in both
modes, in the given and in a shuffled order; the loop of
utils.registration.register_points against the restatement's loop; pose
refinement from ray-cast depth, end to end; argument errors."""
import numpy as np
import pytest
import torch

from tests import register_numpy as RG
from tests.sdf_numpy import broken_mesh, cube, face_unit_normals
from tests.surface_numpy import triangle_grid as numpy_grid
from tests.surface_numpy import valid_faces
from tests.test_gpu_tsdf_fusion import _ops
from tests.test_register_cpu import bits, moved_source, pose_error, rigid, room_mesh, surface_points
from ucsa_neural_rendering_amd.utils import registration as REG

pytestmark = pytest.mark.gpu
F = np.float32


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared references are read-only

TRANSFORMS = {"identity": np.eye(4), "3deg": rigid(3.0, 0.05), "170deg": rigid(170.0, 0.3, seed=3)}
SIZES = {"room": [0, 1, 63, 64, 65, 255, 256, 257, 1000],
         # the brute force over 65 537 points is affordable on 12 faces only
         "box": [256, 1000, 65537],
         "broken": [257, 1000]}


def mesh_of(name):
    if name == "room":
        return room_mesh()
    v, f = cube()[:2] if name == "box" else broken_mesh()
    v, f = np.asarray(v, F), np.asarray(f, np.int32)
    return v, f, face_unit_normals(v, f)


def world_points(v, f, n, seed):
    """``n`` points in the mesh's frame: on the surface, up to 0.3 off it, beyond
    every max_dist, NaN and inf rows, and points exactly on shared edges and
    vertices (ties between faces)"""
    g = np.random.default_rng(seed)
    fv = f[valid_faces(v, f)]
    p = surface_points(v, fv, n, seed).astype(np.float64)
    kind = g.integers(0, 10, n)
    off = g.normal(size=(n, 3))
    off *= (g.uniform(0, 0.3, n) / np.linalg.norm(off, axis=1))[:, None]
    p[kind >= 5] += off[kind >= 5]
    p[kind == 9] += 7.0                                             # beyond max_dist
    p = p.astype(F)
    edge = np.nonzero(kind == 4)[0]
    tri = fv[g.integers(0, fv.shape[0], edge.size)]
    mid = (v[tri[:, 0]] + v[tri[:, 1]]) * F(0.5)                    # on an edge, or a vertex
    p[edge] = np.where((edge % 2 == 0)[:, None], mid, v[tri[:, 2]])
    if n >= 63:
        p[5], p[17, 1], p[40, 2] = np.nan, np.inf, -np.inf
    return p


def source_of(world, T):
    """the points that ``T`` moves onto ``world`` (float32; the identity moves nothing)"""
    if np.array_equal(T, np.eye(4)):
        return world.copy()
    with np.errstate(all="ignore"):
        return ((world.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)


def grids_of(name, v, f):
    """the default cell, a quarter of it and four times it"""
    ops = _ops()
    c = float(numpy_grid(v, f)["cell"])
    vg, fg = _cu(v).view(-1, 3), _cu(f).view(-1, 3)
    return vg, fg, [ops.triangle_grid(vg, fg, cell) for cell in (None, c / 4.0, 4.0 * c)]


@pytest.mark.parametrize("name", sorted(SIZES))
def test_sums_and_matches_equal_the_restatement_byte_for_byte(name):
    ops = _ops()
    v, f, un = mesh_of(name)
    vg, fg, grids = grids_of(name, v, f)
    ung = ops.register.face_unit_normals(vg, fg)
    assert ung.cpu().numpy().tobytes() == un.tobytes()
    checked = 0
    for n in SIZES[name]:
        world = world_points(v, f, n, 100 + n)
        perm = np.random.default_rng(n).permutation(n)
        for tname, T in TRANSFORMS.items():
            if n == 65537 and tname != "3deg":
                continue
            src = source_of(world, T)
            for md in (0.5, 0.05):
                q = RG.transform_points(src, T)
                face, dist2, _ = RG.nearest_triangle(v, f, q, md)
                terms = [RG.point_terms(v, f, un, q, face, mode) for mode in (0, 1)]
                if n >= 256 and md == 0.5:
                    assert (face >= 0).sum() > n // 2, "the case matches too little to test much"
                for order in (None, perm):
                    o = slice(None) if order is None else order
                    pts = _cu(src[o]).view(-1, 3)
                    nt = ops.nearest_triangle(grids[0], _cu(q[o]).view(-1, 3), md)
                    for gi, grid in enumerate(grids):
                        for mode, mname in enumerate(("plane", "point")):
                            want = RG.tree_sum(terms[mode][o])
                            sums, gf, gd = ops.register.icp_sums(grid, vg, fg, ung, pts, T, md, mname,
                                                                 return_matches=True)
                            assert sums.dtype == torch.float64 and tuple(sums.shape) == (29,)
                            where = (name, n, tname, md, order is not None, gi, mname)
                            assert sums.cpu().view(torch.int64).tolist() == bits(want).tolist(), where
                            assert gf.cpu().numpy().tobytes() == face[o].tobytes(), where
                            assert gd.cpu().numpy().tobytes() == dist2[o].tobytes(), where
                            assert torch.equal(gf, nt[0]) and torch.equal(gd.view(torch.int32),
                                                                          nt[1].view(torch.int32))
                            checked += 1
                    again = ops.register.icp_sums(grids[0], vg, fg, ung, pts, T, md, "plane")
                    first = ops.register.icp_sums(grids[0], vg, fg, ung, pts, T, md, "plane")
                    assert torch.equal(again.view(torch.int64), first.view(torch.int64))
    assert checked >= 100


def test_six_iterations_equal_the_restatements_loop():
    v, f, un = room_mesh()
    src, want = moved_source(1000, 3.0, 0.05, seed=8)
    ref_T, ref_hist = RG.register_points(src, v, f, un, max_dist=0.5, iterations=6)
    got = REG.register_points(_cu(src), _cu(v), _cu(f), max_dist=0.5, iterations=6, tol_rot=-1.0,
                              tol_trans=-1.0, sort_points=False)
    assert got["iterations"] == 6 and len(got["history"]) == 6 and got["rank"] == 6
    for k in range(6):
        assert bits(got["history"][k]["sums"]).tolist() == bits(ref_hist[k]).tolist(), k
    assert bits(got["transform"]).tolist() == bits(ref_T).tolist()
    rot, trans = pose_error(got["transform"], want)
    assert rot <= 1e-5 and trans <= 1e-5 and got["matched"] == 1000
    # the sorted order changes the sums' last bits; a transform that differs in its last
    # bits may round to another float32 matrix, which moves the points by float32 spacings
    # (2.4e-7 at a coordinate of 3): the results agree to a few of those, not to the bit
    srt = REG.register_points(_cu(src), _cu(v), _cu(f), max_dist=0.5, iterations=6, tol_rot=-1.0,
                              tol_trans=-1.0)
    assert np.abs(srt["transform"] - ref_T).max() < 1e-6
    dflt = REG.register_points(_cu(src), _cu(v), _cu(f), max_dist=0.5)
    assert dflt["converged"] and dflt["iterations"] < 12
    assert np.abs(dflt["transform"] - ref_T).max() < 1e-6


# the views of the pose test: three of the room's loop poses
VIEWS, H, W = (6, 1, 5), 24, 32


def test_pose_refinement_from_raycast_depth_end_to_end():
    from tests.test_raycast_cpu import room_views
    from ucsa_neural_rendering_amd.utils.mesh_raycast import raycast_views
    v, f, un = room_mesh()
    poses, K = room_views(16, H, W)
    poses = poses[list(VIEWS)]
    mesh = {"verts": v, "faces": f}
    depth = raycast_views(mesh, poses.astype(F), K, H, W, 0.05, 20.0)["depth"]
    for k in range(3):
        true = poses[k].astype(F).astype(np.float64)
        twist = np.concatenate([np.radians(2.0) * np.roll([0.6, -0.64, 0.48], k),
                                0.03 * np.roll([0.48, 0.6, -0.64], k)])
        start = REG.compose(true, twist)
        out = REG.refine_pose(depth[k], start, K, mesh, iterations=10, max_dist=0.3, tol_rot=-1.0,
                              tol_trans=-1.0, sort_points=False)
        pts = REG.backproject(depth[k], K).cpu().numpy()
        assert pts.shape[0] > H * W // 2
        ref_T, ref_hist = RG.register_points(pts, v, f, un, init=start, max_dist=0.3, iterations=10)
        rot, trans = pose_error(ref_T, true)
        print(f"view {VIEWS[k]}: {pts.shape[0]} points, restatement rot {rot:.3e} rad, "
              f"trans {trans:.3e}")
        assert rot <= 1e-4 and trans <= 1e-4, "the restatement misses the bound: choose other views"
        assert out["rank"] == 6 and out["iterations"] == 10
        assert bits(out["pose"]).tolist() == bits(ref_T).tolist()
        rot, trans = pose_error(out["pose"], true)
        assert rot <= 1e-4 and trans <= 1e-4


def test_argument_errors_come_before_the_library(monkeypatch):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    v, f, un = mesh_of("box")
    vg, fg, ung = _cu(v), _cu(f), _cu(un)
    grid = ops.triangle_grid(vg, fg)
    pts = _cu(surface_points(v, f, 10, 0))
    T = np.eye(4)

    def boom(*a, **k):
        raise AssertionError("the op reached lib()")
    monkeypatch.setattr(ops.register, "lib", boom)
    call = ops.register.icp_sums
    bad = [lambda: call(grid, vg.cpu(), fg, ung, pts, T, 0.5),
           lambda: call(grid, vg, fg.cpu(), ung, pts, T, 0.5),
           lambda: call(grid, vg, fg, ung.cpu(), pts, T, 0.5),
           lambda: call(grid, vg, fg, ung, pts.cpu(), T, 0.5),
           lambda: call(grid, vg, fg, ung[:5], pts, T, 0.5),
           lambda: call(grid, vg, fg, ung.reshape(-1), pts, T, 0.5),
           lambda: call(grid, vg, fg, ung, pts, T, 0.0),
           lambda: call(grid, vg, fg, ung, pts, T, -1.0),
           lambda: call(grid, vg, fg, ung, pts, T, float("nan")),
           lambda: call(grid, vg, fg, ung, pts, np.eye(3), 0.5),
           lambda: call(grid, vg, fg, ung, pts, np.zeros(12), 0.5),
           lambda: call(grid, vg, fg, ung, pts, T, 0.5, mode="planes"),
           lambda: call({"records": None}, vg, fg, ung, pts, T, 0.5)]
    for k, c in enumerate(bad):
        with pytest.raises(_lib.UcsaError):
            c()
    monkeypatch.undo()
    # the library's own codes: an argument error comes before any launch
    import ctypes as C
    l = _lib.lib()
    sums = torch.full((29,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def raw(**over):
        a = dict(md=0.5, mode=0, ws=None, wsn=0, sums=sums, n=10, T=(C.c_float * 12)(*T[:3].reshape(-1)))
        a.update(over)
        return l.ucsa_icp_sums(p(grid["records"]), p(grid["offsets"]), grid["n_pairs"],
                               (C.c_float * 3)(*grid["origin"]), grid["cell"],
                               (C.c_uint32 * 3)(*grid["dims"]), p(vg), v.shape[0], p(fg), f.shape[0],
                               p(ung), p(pts), a["n"], a["T"], a["md"], a["mode"], p(a["ws"]),
                               a["wsn"], p(a["sums"]), None, None, None)
    assert raw(md=0.0) == -1014 and raw(mode=2) == -1015 and raw(sums=None) == -1018
    assert raw(T=None) == -1013
    assert raw(n=257) == -1016                       # two groups need a workspace
    torch.cuda.synchronize()
    assert (sums == 7.0).all()
    assert raw() == 0
    torch.cuda.synchronize()
    assert sums[28].item() == 10.0


def test_score_script_registers_before_it_scores(tmp_path, capsys):
    import json

    from scripts import score_mesh_3d
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    v, f, _ = room_mesh()
    T = rigid(3.0, 0.05)
    moved = ((v.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)
    write_ply(str(tmp_path / "p.ply"), moved, np.array(f))
    write_ply(str(tmp_path / "g.ply"), np.array(v), np.array(f))
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply"), "--surface",
            "--max_dist", "0.5", "--threshold", "0.001"]
    capsys.readouterr()
    plain = score_mesh_3d.main(args)
    out = capsys.readouterr().out.splitlines()
    assert out == ["geometry: " + json.dumps(plain["geometry"])] and "register" not in plain
    assert plain["geometry"]["fscore"] < 0.5                       # 3 degrees off: not aligned
    for more in ([], ["--register_samples", "3000"], ["--register_mode", "point",
                                                      "--register_iters", "60"]):
        rec = score_mesh_3d.main(args + ["--register"] + more)
        out = capsys.readouterr().out.splitlines()
        assert out == ["register: " + json.dumps(rec["register"]),
                       "geometry: " + json.dumps(rec["geometry"])]
        reg = rec["register"]
        assert reg["rank"] == 6 and reg["matched"] == 1.0 and reg["iterations"] <= 60
        rot, trans = pose_error(np.array(reg["transform"]), T)
        if "point" not in more:                     # point to point slides: no accuracy gate
            assert rot <= 1e-4 and trans <= 1e-4 and reg["converged"]
            assert rec["geometry"]["fscore"] == 1.0
    with pytest.raises(SystemExit):
        score_mesh_3d.main(args + ["--register", "--register_max_dist", "0"])
