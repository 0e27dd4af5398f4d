"""GPU: TSDF fusion (csrc/tsdf_fusion.hip) and masked marching cubes against the
numpy restatement of their contracts (tests/tsdf_numpy.py), bit for bit; guard
words, argument codes; the scripts end to end from a scene directory:
depth/ + poses -> mesh -> fused labels -> map_label.

The distance bounds are the constants of tests/test_tsdf_fusion_cpu.py.  The
end-to-end figures below were measured with the numpy pipeline (restatement +
tests/raster_numpy.py + tests/fusion_numpy.py) on the same set-up with depth
taken through the uint16-millimetre PNG: 16 views at 240x320, 128^3 volume over
[-3.05, 3.05]^3, trunc = 4 voxels:
  mesh coverage of the pixels with a depth measurement, per view: 0.9891..0.9974
  pixels both see that disagree with the PNG beyond trunc, per view: <= 0.00097
    (beyond one voxel: <= 0.00147)
  label_40 fused onto the TSDF mesh and rendered back: mIoU 0.5341, accuracy
    0.9941 (one class of 4 pixels is lost and the 0.6 % of pixels the mesh does
    not cover count as a class of their own, so two zeros enter the mean of
    five); the same on SyntheticRoom.labelled_mesh(0.1): mIoU 0.9999."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import tsdf_numpy as TN
from tests.test_tsdf_fusion_cpu import (TRUNC_VOXELS, batches, check_distance_bounds,
                                        random_case, room_frames, room_volume_spec,
                                        run_numpy, same_bytes, vertex_distance_voxels,
                                        _smooth_field)

pytestmark = pytest.mark.gpu

GUARD = 1024  # floats before and after each volume
# conditions of the issue, not measurements
DISAGREE_MAX, COVER_MIN = 0.02, 0.98
# 0.02 under the mIoU measured with the numpy pipeline (module docstring)
FUSED_MIOU_MIN = 0.5341 - 0.02


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guarded_volume(dims, origin, spacing, with_color):
    """a volume whose three tensors are views into larger buffers filled with a
    guard pattern -> (volume, check())"""
    nx, ny, nz = dims
    n = nx * ny * nz
    bufs, vol = {}, {"origin": tuple(float(v) for v in origin),
                     "spacing": tuple(float(v) for v in np.broadcast_to(spacing, (3,)))}
    for k, per, init in (("tsdf", 1, 1.0), ("weight", 1, 0.0), ("rgb", 3, 0.0)):
        if k == "rgb" and not with_color:
            vol[k] = None
            continue
        b = torch.full((2 * GUARD + n * per,), -777.25, device="cuda")
        b[GUARD:GUARD + n * per] = init
        bufs[k] = b
        vol[k] = b[GUARD:GUARD + n * per].view((nx, ny, nz) + ((3,) if per == 3 else ()))

    def check():
        for k, b in bufs.items():
            assert (b[:GUARD] == -777.25).all() and (b[-GUARD:] == -777.25).all(), k
    return vol, check


def run_gpu(case, splits, with_color=True):
    ops = _ops()
    vol, check = guarded_volume(case["dims"], case["origin"], case["spacing"], with_color)
    depth, poses, color = _cu(case["depth"]), _cu(case["poses"]), _cu(case["color"])
    for a, b in splits:
        ops.integrate_tsdf(vol, depth[a:b], poses[a:b], case["intr"], case["trunc"],
                           color=color[a:b] if with_color else None,
                           max_weight=case["max_weight"], depth_min=case["depth_min"],
                           depth_max=case["depth_max"])
    torch.cuda.synchronize()
    check()
    return {k: (None if vol[k] is None else vol[k].cpu().numpy())
            for k in ("tsdf", "weight", "rgb")}


def test_random_case_bit_exact_for_every_batch_size_and_twice():
    case = random_case(0, views=16)
    want = run_numpy(case, [(0, 16)])
    assert 0.2 < (want["weight"] > 0).mean() < 1.0 and want["weight"].max() == 11.0
    for size in (1, 5, 16):
        got = run_gpu(case, batches(16, size))
        for k in ("tsdf", "weight", "rgb"):
            assert got[k].tobytes() == want[k].tobytes(), (size, k)
    assert same_bytes(run_gpu(case, [(0, 16)]), want)  # twice in a row
    plain = run_gpu(case, [(0, 16)], with_color=False)
    assert plain["rgb"] is None and plain["tsdf"].tobytes() == want["tsdf"].tobytes()
    assert plain["weight"].tobytes() == want["weight"].tobytes()


def test_more_views_than_one_launch_takes():
    case = random_case(3, views=40)  # 32 views per launch: two launches in one call
    want = run_numpy(case, [(0, 40)])
    assert same_bytes(run_gpu(case, [(0, 40)]), want)


@pytest.fixture(scope="module")
def room_case():
    room, poses, intr, depth = room_frames(240, 320)
    dims, origin, h, trunc = room_volume_spec(128)
    g = np.random.default_rng(11)
    case = {"dims": dims, "origin": np.asarray(origin, np.float32),
            "spacing": np.full(3, h, np.float32), "poses": poses, "depth": depth,
            "color": g.integers(0, 256, depth.shape + (3,)).astype(np.uint8), "intr": intr,
            "trunc": float(trunc), "max_weight": 65504.0, "depth_min": 1e-6,
            "depth_max": 3.0e38}
    return room, case, run_numpy(case, [(0, 16)]), float(h)


def test_room_volume_bit_exact_for_every_batch_size_and_twice(room_case):
    room, case, want, h = room_case
    for size in (1, 5, 16, 16):
        got = run_gpu(case, batches(16, size))
        for k in ("tsdf", "weight", "rgb"):
            assert got[k].tobytes() == want[k].tobytes(), (size, k)


def test_masked_marching_cubes_bit_exact(room_case):
    ops = _ops()
    room, case, vol, h = room_case
    field, valid = -vol["tsdf"], vol["weight"] >= 1
    o, sp = case["origin"], case["spacing"]
    want = TN.marching_cubes_masked(field, 0.0, valid, o, sp)
    got = ops.marching_cubes(_cu(field), 0.0, tuple(o), tuple(sp), valid=_cu(valid))
    assert want[0].shape[0] > 50000
    for a, b in zip(want, got):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    check_distance_bounds(vertex_distance_voxels(room, want[0], h))
    # a random mask over a smooth field, uint8 with values other than 1
    f = _smooth_field(7, (33, 18, 70))
    m = (np.random.default_rng(3).random(f.shape) < 0.85).astype(np.uint8) * 3
    want = TN.marching_cubes_masked(f, 0.05, m, (0.1, 0.2, 0.3), (0.5, 0.25, 0.125))
    got = ops.marching_cubes(_cu(f), 0.05, (0.1, 0.2, 0.3), (0.5, 0.25, 0.125), valid=_cu(m))
    assert want[0].shape[0] > 1000
    for a, b in zip(want, got):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    # all ones: the unmasked entries' bytes
    plain = ops.marching_cubes(_cu(f), 0.05, (0.1, 0.2, 0.3), (0.5, 0.25, 0.125))
    ones = ops.marching_cubes(_cu(f), 0.05, (0.1, 0.2, 0.3), (0.5, 0.25, 0.125),
                              valid=torch.ones(f.shape, dtype=torch.bool, device="cuda"))
    for a, b in zip(plain, ones):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_masked_emit_respects_capacities():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    f = _cu(_smooth_field(7, (33, 18, 70)))
    m = _cu((np.random.default_rng(3).random(tuple(f.shape)) < 0.85).astype(np.uint8))
    nx, ny, nz = f.shape
    ws = torch.empty(int(l.ucsa_mc_workspace_bytes(nx, ny, nz)), dtype=torch.uint8, device="cuda")
    tot = torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert l.ucsa_mc_count_masked(p(f), p(m), nx, ny, nz, 0.05, p(ws), p(tot), None) == 0
    V, F = tot.tolist()
    cv, cf = V // 2, F // 3
    verts = torch.full((V, 3), -5.0, device="cuda")
    normals = torch.full((V, 3), -5.0, device="cuda")
    tris = torch.full((F, 3), -5, dtype=torch.int32, device="cuda")
    o, h = _lib.fvec((0, 0, 0)), _lib.fvec((1, 1, 1))
    assert l.ucsa_mc_emit_masked(p(f), p(m), nx, ny, nz, 0.05, o, h, p(ws), p(verts),
                                 p(normals), p(tris), cv, cf, None) == 0
    torch.cuda.synchronize()
    assert (verts[cv:] == -5).all() and (normals[cv:] == -5).all() and (tris[cf:] == -5).all()
    assert (verts[:cv] != -5).any() and (tris[:cf] >= 0).all()
    # argument codes: valid is argument 1, the dims 2..4
    assert l.ucsa_mc_count_masked(p(f), None, nx, ny, nz, 0.05, p(ws), p(tot), None) == -1001
    assert l.ucsa_mc_count_masked(None, p(m), nx, ny, nz, 0.05, p(ws), p(tot), None) == -1000
    assert l.ucsa_mc_count_masked(p(f), p(m), 1, ny, nz, 0.05, p(ws), p(tot), None) == -1002
    assert l.ucsa_mc_count_masked(p(f), p(m), nx, ny, 1, 0.05, p(ws), p(tot), None) == -1004
    assert l.ucsa_mc_emit_masked(p(f), None, nx, ny, nz, 0.05, o, h, p(ws), p(verts),
                                 p(normals), p(tris), cv, cf, None) == -1001
    assert l.ucsa_mc_emit_masked(p(f), p(m), nx, ny, nz, 0.05, o, None, p(ws), p(verts),
                                 p(normals), p(tris), cv, cf, None) == -1007


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    vol, check = guarded_volume((8, 9, 10), (0, 0, 0), 0.1, True)
    depth = torch.ones(2, 12, 16, device="cuda")
    color = torch.zeros(2, 12, 16, 3, dtype=torch.uint8, device="cuda")
    poses = torch.eye(4, device="cuda").repeat(2, 1, 1).contiguous()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    o, h = _lib.fvec((0, 0, 0)), _lib.fvec((0.1, 0.1, 0.1))
    base = dict(tsdf=p(vol["tsdf"]), weight=p(vol["weight"]), rgb=p(vol["rgb"]), nx=8, ny=9,
                nz=10, origin=o, spacing=h, depth=p(depth), color=p(color), poses=p(poses), B=2,
                fx=10.0, fy=10.0, cx=8.0, cy=6.0, H=12, W=16, trunc=0.3, max_weight=10.0,
                depth_min=0.01, depth_max=5.0, stream=None)

    def rc(**kw):
        return l.ucsa_tsdf_integrate(*{**base, **kw}.values())

    before = {k: vol[k].clone() for k in ("tsdf", "weight", "rgb")}
    for kw, code in ((dict(tsdf=None), 0), (dict(weight=None), 1), (dict(rgb=None), 2),
                     (dict(color=None), 9), (dict(nx=1), 3), (dict(ny=1), 4), (dict(nz=1), 5),
                     (dict(nx=2048, ny=2048, nz=2048), 3), (dict(origin=None), 6),
                     (dict(spacing=None), 7), (dict(depth=None), 8), (dict(poses=None), 10),
                     (dict(B=0), 11), (dict(fx=0.0), 12), (dict(fy=-1.0), 13),
                     (dict(H=0), 16), (dict(H=16385), 16), (dict(W=16385), 17),
                     (dict(trunc=0.0), 18), (dict(trunc=float("nan")), 18),
                     (dict(max_weight=0.5), 19), (dict(depth_min=float("nan")), 20),
                     (dict(depth_max=0.001), 21)):
        assert rc(**kw) == -1000 - code, (kw, code)
    torch.cuda.synchronize()
    check()
    for k in before:
        assert torch.equal(vol[k], before[k])  # an argument error launches nothing
    assert rc() == 0 and rc(rgb=None, color=None) == 0
    torch.cuda.synchronize()
    check()
    assert (vol["weight"] > 0).any()
    # ops
    intr = (10.0, 10.0, 8.0, 6.0)
    v = ops.tsdf_volume((8, 9, 10), (0, 0, 0), 0.1, with_color=False)
    assert v["rgb"] is None and (v["tsdf"] == 1).all() and (v["weight"] == 0).all()
    with pytest.raises(UcsaError):
        ops.tsdf_volume((1, 9, 10), (0, 0, 0), 0.1)
    with pytest.raises(UcsaError):
        ops.tsdf_volume((8, 9, 10), (0, 0, 0), 0.1, device="cpu")
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth.cpu(), poses, intr, 0.3)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth, poses.cpu(), intr, 0.3)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf({**v, "tsdf": v["tsdf"].cpu()}, depth, poses, intr, 0.3)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth, poses, intr, 0.3, color=color)  # no colour volume
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth, poses[:1], intr, 0.3)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth, poses, intr, 0.0)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(v, depth, poses, intr, 0.3, max_weight=0.0)
    vc = ops.tsdf_volume((8, 9, 10), (0, 0, 0), 0.1, with_color=True)
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(vc, depth, poses, intr, 0.3, color=color.cpu())
    with pytest.raises(UcsaError):
        ops.integrate_tsdf(vc, depth, poses, intr, 0.3, color=color.float())
    f = torch.zeros(4, 4, 4, device="cuda")
    with pytest.raises(UcsaError):
        ops.marching_cubes(f, 0.0, valid=torch.ones(4, 4, 4, dtype=torch.bool))
    with pytest.raises(UcsaError):
        ops.marching_cubes(f, 0.0, valid=torch.ones(4, 4, 5, dtype=torch.bool, device="cuda"))
    with pytest.raises(UcsaError):
        ops.marching_cubes(f, 0.0, valid=torch.ones(4, 4, 4, device="cuda"))
    assert ops.integrate_tsdf(v, depth, poses, intr, 0.3) is v


def test_fuse_depth_views_picks_the_volume_and_colours_the_mesh():
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import fuse_depth_views
    room, poses, intr, depth = room_frames(120, 160, views=8)
    col = np.zeros((8, 120, 160, 3), np.uint8)
    col[..., 0], col[..., 1], col[..., 2] = 40, 120, 200
    mesh = fuse_depth_views(poses, intr, 120, 160, lambda i: depth[i], color_maps=col,
                            voxel=0.08, batch=3)
    trunc = 4 * 0.08
    # the box of the back-projected depth points, padded by trunc
    fx, fy, cx, cy = intr
    ys, xs = np.mgrid[0:120, 0:160].astype(np.float64)
    ray = np.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, np.ones_like(xs)], -1)
    pts = np.concatenate([(ray * depth[b][..., None].astype(np.float64)).reshape(-1, 3)
                          @ poses[b, :3, :3].astype(np.float64).T + poses[b, :3, 3]
                          for b in range(8)])
    lo = np.asarray(mesh["origin"])
    hi = lo + (np.asarray(mesh["dims"]) - 1) * np.asarray(mesh["spacing"])
    assert np.abs(lo - (pts.min(0) - trunc)).max() < 1e-3
    assert np.all(hi >= pts.max(0) + trunc - 1e-3) and np.all(hi <= pts.max(0) + trunc + 0.081)
    assert mesh["faces"].dtype == np.int32 and mesh["verts"].shape[0] > 5000
    assert mesh["faces"].max() < mesh["verts"].shape[0] and mesh["labels"] is None
    want = np.array([40, 120, 200], np.float32) / 255.0
    assert np.abs(mesh["rgb"] - want).max() < 1e-5
    # whatever the volume: a vertex lies within trunc + one voxel of the room
    assert vertex_distance_voxels(room, mesh["verts"], 0.08).max() <= TRUNC_VOXELS + 1.0
    assert np.all(mesh["verts"] >= lo - 1e-4) and np.all(mesh["verts"] <= hi + 1e-4)
    assert mesh["integrate_ms"] > 0 and mesh["extract_ms"] > 0


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_scripts_end_to_end_from_a_scene_directory(tmp_path, capsys):
    from scripts import fuse_mesh_labels, fuse_tsdf_mesh
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.mesh_render import load_mesh
    from ucsa_neural_rendering_amd.utils.ply import read_ply, write_ply
    ops = _ops()
    H, W, n = 240, 320, 16
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=H, W=W)
    dims, origin, h, trunc = room_volume_spec(128)
    out = str(tmp_path / "mesh" / "tsdf.ply")
    rec = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", out, "--voxel", repr(float(h)),
                               "--aabb", "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == n and line["dims"] == [128, 128, 128]
    assert line["vertices"] == rec["vertices"] > 50000 and line["integrate_ms_per_view"] > 0
    ply = read_ply(out)
    assert ply["verts"].shape == (rec["vertices"], 3) and ply["faces"].shape[0] == rec["faces"]
    assert "normals" in ply and ply["rgb"].dtype == np.uint8 and "labels" not in ply
    d = vertex_distance_voxels(ds.room.to("cpu"), ply["verts"], h)
    ds.room.to("cuda")
    with capsys.disabled():
        print(f"\nTSDF mesh: {rec['vertices']} vertices, distance in voxels median "
              f"{np.median(d):.4f}, p95 {np.percentile(d, 95):.4f}, max {d.max():.4f}; "
              f"integrate {rec['integrate_ms_per_view']} ms/view, extract {rec['extract_ms']} ms")
    check_distance_bounds(d)
    # the mesh against the depth it was made from
    mesh = load_mesh(out)
    z = ops.rasterize_mesh(_cu(mesh["verts"]), _cu(mesh["faces"]), ds.poses.float(),
                           ds.intrinsics.tolist(), H, W, 0.05)["depth"].cpu().numpy()
    tol = float(TRUNC_VOXELS * h)
    for b in range(n):
        png = (_png(os.path.join(sroot, "depth", f"{b:06d}.png")).astype(np.float32) /
               np.float32(1000.0)) * np.float32(1.0)
        have = png > 0
        both = have & (z[b] > 0)
        cover = both.sum() / have.sum()
        off = (np.abs(z[b][both] - png[both]) > tol).mean()
        with capsys.disabled():
            print(f"view {b}: covered {cover:.5f}, beyond trunc {off:.5f}")
        assert cover >= COVER_MIN
        assert off <= DISAGREE_MAX
    # the chain the README promises: labels fused onto that mesh and rendered back
    fused = str(tmp_path / "mesh" / "tsdf.labels.ply")
    capsys.readouterr()
    fuse_mesh_labels.main(["--scene_root", sroot, "--mesh", out, "--labels", "label_40",
                           "--out", fused, "--score", "--out_dir", str(tmp_path / "maps")])
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (read_ply(fused)["labels"] > 0).mean() > 0.9
    # the parent's route: the analytic room's own geometry
    m = ds.room.labelled_mesh(0.1)
    analytic = str(tmp_path / "mesh" / "room.ply")
    write_ply(analytic, m["verts"], m["faces"])
    fuse_mesh_labels.main(["--scene_root", sroot, "--mesh", analytic, "--labels", "label_40",
                           "--out", str(tmp_path / "mesh" / "room.labels.ply"), "--score",
                           "--out_dir", str(tmp_path / "maps_room")])
    ref = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    with capsys.disabled():
        print(f"fused mIoU on the TSDF mesh {got['fused']['mIoU']:.4f} (accuracy "
              f"{got['fused']['total_acc']:.4f}); on SyntheticRoom.labelled_mesh(0.1) "
              f"{ref['fused']['mIoU']:.4f} (accuracy {ref['fused']['total_acc']:.4f})")
    assert got["fused"]["mIoU"] >= FUSED_MIOU_MIN
    # --pose_frame writes what fuse_mesh_labels.py --pose_frame reads back
    box = ["--voxel", repr(float(h)), "--aabb", "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05"]
    out_pf = str(tmp_path / "mesh" / "tsdf_pf.ply")
    fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", out_pf, "--pose_frame", "--no_color"]
                        + box)
    back = load_mesh(out_pf, pose_frame=True, one_m_to_scene_uom=1.0)
    assert "rgb" not in read_ply(out_pf)
    assert np.array_equal(back["verts"], mesh["verts"])
    assert np.array_equal(back["faces"], mesh["faces"])
    # fewer frames and a higher observation count: a smaller mesh
    few = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "few.ply"),
                               "--every", "2", "--min_weight", "2", "--no_color"] + box)
    assert few["frames"] == n // 2 and 0 < few["vertices"] < rec["vertices"]
