"""GPU: the ICP step against a TSDF volume (csrc/mesh_register.hip:
ucsa_tsdf_icp_sums; ops.register.tsdf_sums) against the restatement of
tests/tsdf_register_numpy.py, byte for byte: the 29 sums as int64 words, the
values as int32 words (NaNs included), the matches; the loop of
utils.registration.register_points_tsdf against the restatement's loop; pose
refinement against fused views of SyntheticRoom, end to end; frame-to-model
tracking inside fuse_depth_views under a smooth drift and with a frame that
falls back; argument errors; the script.  The inputs and the gates are those
of tests/test_tsdf_register_cpu.py (figures: docs/DESIGN_NOTEBOOK.md, TR)."""
import json

import numpy as np
import pytest
import torch

from tests import tsdf_register_numpy as TR
from tests.test_gpu_tsdf_fusion import _ops
from tests.test_register_cpu import bits, pose_error, rigid
from tests.test_tsdf_register_cpu import (HELD_OUT_GATE_ROT, HELD_OUT_GATE_TRANS,
                                          HELD_OUT_ITERATIONS, ROOM_TRUNC, SR_H, SR_HELD, SR_VIEWS,
                                          SR_W, drifted_poses, held_out_start, median_distance,
                                          room_points, room_volume, synthetic_case, twist,
                                          two_wall_view)
from ucsa_neural_rendering_amd.utils import registration as REG

pytestmark = pytest.mark.gpu
F = np.float32


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared references are read-only


def gpu_volume(vol):
    """a numpy volume (tests/tsdf_numpy.py) as ``ops.tsdf_volume`` gives it"""
    return {"tsdf": _cu(vol["tsdf"]), "weight": _cu(vol["weight"]), "rgb": None,
            "origin": tuple(float(v) for v in np.asarray(vol["origin"], F)),
            "spacing": tuple(float(v) for v in np.broadcast_to(np.asarray(vol["spacing"], F), 3))}


# ---- the step ---------------------------------------------------------------------
VOLUMES = {"small": ((9, 10, 11), (0.1, 0.07, 0.13), (-0.35, 0.4, -0.6)),
           "odd": ((33, 20, 17), (0.05, 0.06, 0.055), (-0.9, 0.4, -0.4))}
SIZES = [0, 1, 255, 256, 257, 65537]            # 65 537: three reduce stages
TRANSFORMS = {"identity": np.eye(4), "3deg": rigid(3.0, 0.05), "170deg": rigid(170.0, 0.3, seed=3)}


def random_volume(name):
    """a smooth field clamped to [-1, 1] (so that whole cells sit at +1 and -1),
    weights 0..3 at random with unobserved clumps"""
    dims, spacing, origin = VOLUMES[name]
    g = np.random.default_rng(len(name))
    i, j, k = np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij")
    f = 1.6 * np.sin(0.55 * i + 0.3) * np.cos(0.45 * j - 0.2) + 0.9 * np.sin(0.5 * k + 0.1 * i)
    tsdf = np.clip(f + g.normal(0, 0.02, dims), -1.0, 1.0).astype(F)
    weight = g.integers(1, 4, dims).astype(F)
    weight[g.random(dims) < 0.03] = 0.0
    weight[dims[0] // 2:dims[0] // 2 + 2, 2:5, 3:6] = 0.0
    return {"tsdf": tsdf, "weight": weight, "rgb": None, "origin": np.asarray(origin, F),
            "spacing": np.asarray(spacing, F)}


def world_points(vol, n, seed):
    """``n`` float32 points in the volume's frame: inside, outside, exactly on the six
    faces and the eight corners of the lattice's box, in cells with an unobserved
    corner, in constant cells, NaN and inf rows"""
    g = np.random.default_rng(seed)
    dims = np.array(vol["tsdf"].shape)
    o, h = vol["origin"].astype(np.float64), vol["spacing"].astype(np.float64)
    top = (vol["origin"] + (dims - 1).astype(F) * vol["spacing"]).astype(F)
    ext = (dims - 1) * h
    p = (o + g.uniform(0, 1, (n, 3)) * ext).astype(F)
    kind = g.integers(0, 12, n)
    out = kind == 0                                                   # outside, up to half a box
    p[out] += (np.sign(g.normal(size=(out.sum(), 3))) * g.uniform(0, 0.5, (out.sum(), 3))
               * ext * (g.random((out.sum(), 3)) < 0.5)).astype(F)
    for r in np.nonzero(kind == 1)[0]:                                # on a face
        a = g.integers(0, 3)
        p[r, a] = (vol["origin"], top)[g.integers(0, 2)][a]
    for r in np.nonzero(kind == 2)[0]:                                # on a corner
        pick = g.integers(0, 2, 3)
        p[r] = np.where(pick == 0, vol["origin"], top)
    dark = np.argwhere(vol["weight"] == 0)
    flat = np.argwhere(np.abs(vol["tsdf"]) == 1)
    for code, cells in ((3, dark), (4, flat)):
        rows = np.nonzero(kind == code)[0]
        c = cells[g.integers(0, len(cells), rows.size)]
        p[rows] = (o + (c + g.uniform(-1, 1, (rows.size, 3))) * h).astype(F)
    if n >= 255:
        p[5], p[17, 1], p[40, 2], p[41] = np.nan, np.inf, -np.inf, np.inf
    return p


def source_of(world, T):
    if np.array_equal(T, np.eye(4)):
        return world.copy()
    with np.errstate(all="ignore"):
        return ((world.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_sums_values_and_matches_equal_the_restatement_byte_for_byte(name):
    ops = _ops()
    vol = random_volume(name)
    gvol = gpu_volume(vol)
    trunc = 0.3
    checked, seen = 0, {"unobserved": 0, "flat": 0, "gated": 0, "outside": 0, "matched": 0}
    for n in SIZES:
        world = world_points(vol, n, 200 + n)
        perm = np.random.default_rng(n).permutation(n)
        for tname, T in TRANSFORMS.items():
            if n == 65537 and tname == "170deg":
                continue
            src = source_of(world, T)
            for min_weight in (1.0, 2.0):
                for max_tsdf in (1.0, 0.5):
                    q = TR.transform_points(src, T)
                    matched, J, r, value = TR.point_rows(vol, q, trunc, min_weight, max_tsdf)
                    terms = TR.point_terms(matched, J, r)
                    s = TR.sample(vol, q, min_weight)
                    seen["outside"] += int((~s["inside"]).sum())
                    seen["unobserved"] += int((s["inside"] & ~s["observed"]).sum())
                    seen["flat"] += int((s["observed"] & (s["ln"] == 0)).sum())
                    seen["gated"] += int((s["observed"] & (s["ln"] > 0) & ~matched).sum())
                    seen["matched"] += int(matched.sum())
                    for order in (None, perm):
                        o = slice(None) if order is None else order
                        pts = _cu(src[o]).view(-1, 3)
                        want = TR.tree_sum(terms[o])
                        sums, gv, gm = ops.register.tsdf_sums(gvol, pts, T, trunc, min_weight,
                                                              max_tsdf, return_matches=True)
                        where = (name, n, tname, min_weight, max_tsdf, order is not None)
                        assert sums.dtype == torch.float64 and tuple(sums.shape) == (29,)
                        assert gv.dtype == torch.float32 and gm.dtype == torch.uint8
                        assert sums.cpu().view(torch.int64).tolist() == bits(want).tolist(), where
                        assert gv.cpu().numpy().view(np.int32).tolist() == \
                            value[o].view(np.int32).tolist(), where
                        assert gm.cpu().numpy().tobytes() == \
                            matched[o].astype(np.uint8).tobytes(), where
                        again = ops.register.tsdf_sums(gvol, pts, T, trunc, min_weight, max_tsdf)
                        assert torch.equal(again.view(torch.int64), sums.view(torch.int64)), where
                        checked += 1
    assert checked >= 130
    assert all(v > 100 for v in seen.values()), seen     # every kind of row was there
    assert torch.equal(gvol["tsdf"].cpu(), torch.from_numpy(vol["tsdf"]))   # inputs untouched
    assert torch.equal(gvol["weight"].cpu(), torch.from_numpy(vol["weight"]))


def test_the_lattice_faces_match_and_one_ulp_outside_does_not():
    from tests.test_tsdf_register_cpu import FACE, face_points, face_volume
    ops = _ops()
    vol = face_volume()
    gvol = gpu_volume(vol)
    for pts, want in zip(face_points(), (1, 0, 1)):
        ref = TR.tsdf_sums(vol, pts, np.eye(4), FACE["trunc"])
        sums, gv, gm = ops.register.tsdf_sums(gvol, _cu(pts), np.eye(4), FACE["trunc"],
                                              return_matches=True)
        assert (gm.cpu().numpy() == want).all() and sums[28].item() == want * len(pts)
        assert sums.cpu().view(torch.int64).tolist() == bits(ref[0]).tolist()
        assert gv.cpu().numpy().view(np.int32).tolist() == ref[1].view(np.int32).tolist()


# ---- the loop -----------------------------------------------------------------------
def test_six_iterations_equal_the_restatements_loop():
    vol = room_volume()
    pts = room_points(1000, 11)
    start = REG.compose(np.eye(4), twist(3.0, 0.05, 0))
    kw = dict(init=start, iterations=6, tol_rot=-1.0, tol_trans=-1.0)
    ref = TR.register_points_tsdf(pts, vol, ROOM_TRUNC, **kw)
    got = REG.register_points_tsdf(_cu(pts), gpu_volume(vol), ROOM_TRUNC, **kw)
    assert got["iterations"] == 6 and len(got["history"]) == 6 and got["rank"] == 6
    for k in range(6):
        assert bits(got["history"][k]["sums"]).tolist() == bits(ref["history"][k]["sums"]).tolist(), k
    assert bits(got["transform"]).tolist() == bits(ref["transform"]).tolist()
    assert sorted(got) == ["converged", "history", "iterations", "matched", "n_points", "rank",
                           "rmse", "transform"]             # register_points' keys
    assert got["matched"] == 1000 and got["n_points"] == 1000
    # the schedule is indexed like max_dist_schedule
    sch = REG.register_points_tsdf(_cu(pts), gpu_volume(vol), ROOM_TRUNC, init=start, iterations=4,
                                   max_tsdf_schedule=[1.0, 0.5], tol_rot=-1.0, tol_trans=-1.0)
    assert [h["max_tsdf"] for h in sch["history"]] == [1.0, 0.5, 0.5, 0.5]
    # the default tolerances, on the inputs the gate of section TR was measured with
    dflt = REG.register_points_tsdf(_cu(room_points(600, 7)), gpu_volume(vol), ROOM_TRUNC,
                                    init=REG.compose(np.eye(4), twist(2.0, 0.03, 0)))
    rot, trans = pose_error(dflt["transform"], np.eye(4))
    from tests.test_tsdf_register_cpu import LOOP_GATE_ROT, LOOP_GATE_TRANS
    assert dflt["converged"] and dflt["iterations"] <= 15
    assert rot <= LOOP_GATE_ROT and trans <= LOOP_GATE_TRANS


# ---- end to end on fused views ---------------------------------------------------------
def fuse_on_gpu(case, views, depth=None, poses=None):
    ops = _ops()
    vol = ops.tsdf_volume(case["dims"], list(case["origin"]), case["h"], device="cuda")
    d = case["depth"] if depth is None else depth
    P = case["poses"] if poses is None else poses
    ops.integrate_tsdf(vol, _cu(d[views]), _cu(np.asarray(P, F)[views]), case["intr"], case["trunc"])
    return vol


def numpy_volume(gvol):
    return {"tsdf": gvol["tsdf"].cpu().numpy(), "weight": gvol["weight"].cpu().numpy(),
            "rgb": None, "origin": np.asarray(gvol["origin"], F),
            "spacing": np.asarray(gvol["spacing"], F)}


def test_pose_refinement_against_fused_views_end_to_end():
    case = synthetic_case()
    gvol = fuse_on_gpu(case, [i for i in range(SR_VIEWS) if i != SR_HELD])
    vol = numpy_volume(gvol)
    depth = _cu(case["depth"][SR_HELD])
    pts = REG.backproject(depth, case["intr"]).cpu().numpy()
    assert pts.shape[0] > SR_H * SR_W // 2
    kw = dict(iterations=HELD_OUT_ITERATIONS, tol_rot=-1.0, tol_trans=-1.0)
    for seed in (0, 3):
        true, start = held_out_start(case, seed)
        out = REG.refine_pose_tsdf(depth, start, case["intr"], gvol, case["trunc"], **kw)
        ref = TR.register_points_tsdf(pts, vol, case["trunc"], init=start, **kw)
        assert bits(out["pose"]).tolist() == bits(ref["transform"]).tolist()
        assert out["pose"] is out["transform"] and out["rank"] == 6
        rot, trans = pose_error(out["pose"], true)
        print(f"seed {seed}: rot {rot:.4e} rad (gate {HELD_OUT_GATE_ROT:.3e}), trans "
              f"{trans:.4e} (gate {HELD_OUT_GATE_TRANS:.3e})")
        assert rot <= HELD_OUT_GATE_ROT and trans <= HELD_OUT_GATE_TRANS
    # two walls: the shift along their edge is free and stays
    ops = _ops()
    P, z, start = two_wall_view(case)
    gv2 = ops.tsdf_volume(case["dims"], list(case["origin"]), case["h"], device="cuda")
    ops.integrate_tsdf(gv2, _cu(z[None]), _cu(P[None]), case["intr"], case["trunc"])
    out = REG.refine_pose_tsdf(_cu(z), start, case["intr"], gv2, case["trunc"], iterations=10,
                               tol_rot=-1.0, tol_trans=-1.0)
    ref = TR.register_points_tsdf(REG.backproject(_cu(z), case["intr"]).cpu().numpy(),
                                  numpy_volume(gv2), case["trunc"], init=start, iterations=10,
                                  tol_rot=-1.0, tol_trans=-1.0)
    assert out["rank"] == 5 and bits(out["pose"]).tolist() == bits(ref["transform"]).tolist()
    dz = out["pose"][2, 3] - float(P[2, 3])
    assert 0.9 * 0.03 <= dz <= 1.1 * 0.03


# ---- tracking inside the fusion ----------------------------------------------------------
BOX = [-3.05] * 3 + [3.05] * 3


def test_tracking_under_a_smooth_drift_beats_the_drifted_fusion():
    """measured on the MI355X: median vertex distance to the analytic room 0.02046
    units with the drifted poses as given, 0.01212 with refine_poses=True, 0.00552 with
    the true poses (the floor); no fallback in 15 refined frames"""
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import extract_mesh, fuse_depth_views
    case = synthetic_case()
    drifted = drifted_poses(case)
    kw = dict(aabb=BOX, voxel=case["h"], trunc=case["trunc"])
    args = (case["intr"], SR_H, SR_W, case["depth"])
    plain = fuse_depth_views(drifted, *args, refine_poses=False, **kw)
    refined = fuse_depth_views(drifted, *args, refine_poses=True,
                               refine_kw={"iterations": HELD_OUT_ITERATIONS}, **kw)
    true = fuse_depth_views(case["poses"], *args, **kw)
    assert plain["dims"] == refined["dims"] == tuple(case["dims"])
    assert "poses" not in plain and "refine" not in plain
    med = {k: median_distance(case, m["verts"]) for k, m in
           (("drifted", plain), ("refined", refined), ("true", true))}
    print(f"median vertex distance to the room, units: drifted {med['drifted']:.5f}, refined "
          f"{med['refined']:.5f}, true poses (the floor) {med['true']:.5f}")
    assert med["refined"] < med["drifted"]
    recs = refined["refine"]
    assert len(recs) == SR_VIEWS and recs[0] is None
    assert sum(r["fallback"] for r in recs[1:]) == 0
    assert all(r["rank"] == 6 and 0.25 <= r["matched"] <= 1.0 for r in recs[1:])
    assert refined["poses"].shape == (SR_VIEWS, 4, 4) and refined["poses"].dtype == np.float64
    assert np.array_equal(refined["poses"][0], drifted[0].astype(np.float64))
    # refine_poses=False is the fusion as it was: one batched integration and the extraction
    gvol = fuse_on_gpu(case, list(range(SR_VIEWS)), poses=drifted)
    v, f, _, _ = extract_mesh(gvol, 1)
    assert plain["verts"].tobytes() == v.cpu().numpy().tobytes()
    assert plain["faces"].tobytes() == f.cpu().numpy().tobytes()


def test_a_frame_that_falls_back_keeps_its_pose_and_is_integrated_and_counted():
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import track_depth_views
    ops = _ops()
    case = synthetic_case()
    depth = np.array(case["depth"][:3])
    patch = np.zeros_like(depth[2])
    patch[0:6, 0:8] = depth[2][0:6, 0:8]              # a corner of the image: one wall
    depth[2] = patch
    weights = []
    for n in (2, 3):
        vol = ops.tsdf_volume(case["dims"], list(case["origin"]), case["h"], device="cuda")
        out = track_depth_views(vol, case["poses"][:n], case["intr"], SR_H, SR_W, depth[:n],
                                case["trunc"], refine_kw={"iterations": 5})
        weights.append(float(vol["weight"].sum()))
    recs = out["refine"]
    print("the patch frame:", recs[2])
    assert recs[2]["fallback"] and not recs[1]["fallback"]
    assert sum(bool(r and r["fallback"]) for r in recs) == 1
    assert np.array_equal(out["poses"][2], case["poses"][2].astype(np.float64))
    assert weights[1] > weights[0]                    # integrated all the same


# ---- arguments ---------------------------------------------------------------------------
def test_argument_errors_come_before_the_library(monkeypatch):
    import ctypes as C

    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    vol = gpu_volume(random_volume("small"))
    pts = _cu(world_points(random_volume("small"), 10, 0))
    T = np.eye(4)

    def boom(*a, **k):
        raise AssertionError("the op reached lib()")
    monkeypatch.setattr(ops.register, "lib", boom)
    call = ops.register.tsdf_sums
    bad = [lambda: call(vol, pts.cpu(), T, 0.3),
           lambda: call({**vol, "tsdf": vol["tsdf"].cpu()}, pts, T, 0.3),
           lambda: call({**vol, "weight": vol["weight"][:-1]}, pts, T, 0.3),
           lambda: call({**vol, "spacing": (0.1, 0.0, 0.1)}, pts, T, 0.3),
           lambda: call({**vol, "origin": (0.0, float("nan"), 0.0)}, pts, T, 0.3),
           lambda: call(vol, pts.double(), T, 0.3),
           lambda: call(vol, pts[:, :2], T, 0.3),
           lambda: call(vol, pts.reshape(-1), T, 0.3),
           lambda: call(vol, pts, np.eye(3), 0.3),
           lambda: call(vol, pts, np.zeros(12), 0.3),
           lambda: call(vol, pts, T, 0.0),
           lambda: call(vol, pts, T, float("nan")),
           lambda: call(vol, pts, T, 0.3, min_weight=0.0),
           lambda: call(vol, pts, T, 0.3, min_weight=float("nan")),
           lambda: call(vol, pts, T, 0.3, max_tsdf=0.0),
           lambda: call(vol, pts, T, 0.3, max_tsdf=1.5),
           lambda: call({**vol, "tsdf": vol["tsdf"][:1].contiguous(),
                         "weight": vol["weight"][:1].contiguous()}, pts, T, 0.3)]
    for k, c in enumerate(bad):
        with pytest.raises(_lib.UcsaError):
            c()
    monkeypatch.undo()
    # the library's own codes: an argument error comes before any launch
    l = _lib.lib()
    sums = torch.full((29,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f3 = lambda v: (C.c_float * 3)(*v)

    def raw(**over):
        a = dict(tsdf=vol["tsdf"], dims=(9, 10, 11), origin=f3(vol["origin"]),
                 spacing=f3(vol["spacing"]), n=10, T=(C.c_float * 12)(*T[:3].reshape(-1)),
                 trunc=0.3, mw=1.0, mt=1.0, ws=None, wsn=0, sums=sums)
        a.update(over)
        return l.ucsa_tsdf_icp_sums(p(a["tsdf"]), p(vol["weight"]), *a["dims"], a["origin"],
                                    a["spacing"], p(pts), a["n"], a["T"], a["trunc"], a["mw"],
                                    a["mt"], p(a["ws"]), a["wsn"], p(a["sums"]), None, None, None)
    assert raw(tsdf=None) == -1000 and raw(dims=(1, 10, 11)) == -1002
    assert raw(dims=(9, 1, 11)) == -1003 and raw(dims=(9, 10, 1)) == -1004
    assert raw(dims=(2048, 2048, 2048)) == -1002
    assert raw(origin=f3((0.0, float("inf"), 0.0))) == -1005
    assert raw(spacing=f3((0.1, -0.1, 0.1))) == -1006 and raw(T=None) == -1009
    assert raw(trunc=0.0) == -1010 and raw(mw=0.0) == -1011 and raw(mt=1.5) == -1012
    assert raw(n=257) == -1013 and raw(sums=None) == -1015
    torch.cuda.synchronize()
    assert (sums == 7.0).all()
    assert raw() == 0
    torch.cuda.synchronize()
    ref = TR.tsdf_sums(random_volume("small"), pts.cpu().numpy(), T, 0.3)[0]
    assert sums.cpu().view(torch.int64).tolist() == bits(ref).tolist()


# ---- the script ----------------------------------------------------------------------------
def test_script_refines_poses_and_is_unchanged_without_the_flag(tmp_path, capsys):
    from scripts import fuse_tsdf_mesh
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=12, H=48, W=64)
    box = ["--voxel", "0.1", "--aabb"] + [str(v) for v in BOX] + ["--no_color"]
    capsys.readouterr()
    plain = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "a.ply")] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == plain
    assert sorted(plain) == ["dims", "extract_ms", "faces", "frames", "integrate_ms_per_view",
                             "observed", "origin", "out", "vertices", "voxel"]
    again = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "b.ply")] + box)
    capsys.readouterr()
    a, b = read_ply(str(tmp_path / "a.ply")), read_ply(str(tmp_path / "b.ply"))
    assert a["verts"].tobytes() == b["verts"].tobytes() and again["faces"] == plain["faces"]
    out = str(tmp_path / "poses" / "used.npy")
    rec = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "c.ply"),
                               "--refine_poses", "--refine_iters", "10", "--refine_stride", "2",
                               "--poses_out", out] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("refine: ")
    line = json.loads(lines[0][len("refine: "):])
    assert line == rec["refine"] and line["refined"] == 11 and 0 <= line["fallbacks"] <= 11
    assert sorted(line) == ["fallbacks", "refined", "rmse_median", "step_rad_max",
                            "step_rad_median", "step_units_max", "step_units_median"]
    poses = np.load(out)
    assert poses.shape == (12, 4, 4) and poses.dtype == np.float64
    assert read_ply(str(tmp_path / "c.ply"))["verts"].shape[0] > 1000
    with pytest.raises(SystemExit):
        fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "d.ply"),
                             "--poses_out", out] + box)
