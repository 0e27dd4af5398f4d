"""GPU: label fusion (csrc/label_fusion.hip, ops.fuse_label_votes /
ops.resolve_label_votes, utils/mesh_fusion.py, scripts/fuse_mesh_labels.py).

- The vote table and label / total / winner BIT-identical to the numpy
  restatement (tests/fusion_numpy.py) on the seeded triangle soup and on the
  analytic room at a fine and a coarse grid step and two sizes, with random and
  with coherent (clean-render) predictions, with and without weights and the
  depth gate; several calls equal one call; two runs give the same bytes; the
  one-atomic-per-pixel form gives the same table.
- A cell that passes 2^32.
- Capacity and guard words through ctypes, argument errors, empty inputs.
- utils/mesh_fusion.fuse_views equals the CPU restatement pipeline.
- scripts/fuse_mesh_labels.py end to end on an exported synthetic scene."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import fusion_numpy as FN
from tests import raster_numpy as R
from tests.test_gpu_mesh_raster import _soup
from tests.test_label_fusion_cpu import (HELD_OUT_AGREE_MIN, ROOM_H, ROOM_W, noisy_labels,
                                         room_setup)
from tests.test_mesh_raster_cpu import room_views

pytestmark = pytest.mark.gpu

NC = 40


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _cu(a, dt=None):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a, dt))).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _ids_and_depth(verts, faces, poses, intr, H, W, labels=None):
    """the rasterizer's vote targets (bit-identical to tests/raster_numpy.py:
    tests/test_gpu_mesh_raster.py), its depth, and the clean label render"""
    ops = _ops()
    V = verts.shape[0]
    v, f, p = _cu(verts, np.float32), _cu(faces, np.int32), _cu(poses, np.float32)
    out = ops.rasterize_mesh(v, f, p, intr, H, W, 0.05,
                             vertex_labels=torch.arange(1, V + 1, dtype=torch.int32,
                                                        device="cuda"))
    clean = None
    if labels is not None:
        clean = ops.rasterize_mesh(v, f, p, intr, H, W, 0.05,
                                   vertex_labels=_cu(labels, np.int32))["label"]
        clean = clean.clamp(0, 255).to(torch.uint8)
    return out["label"], out["depth"], clean


def _check_variants(V, vid, depth, clean, seed):
    """every variant of one (mesh, views) case against the restatement"""
    ops = _ops()
    g = np.random.default_rng(seed)
    shape = tuple(vid.shape)
    vid_np = vid.cpu().numpy()
    md_np = depth.cpu().numpy()
    preds = {"random": g.integers(0, NC + 3, shape).astype(np.uint8)}
    if clean is not None:
        preds["clean"] = clean.cpu().numpy()
    w_np = g.integers(0, 65536, shape).astype(np.int32)
    w_np[..., ::5] = 65535
    w_np[..., 1::9] = 0
    sd_np = (md_np + g.normal(0, 0.01, shape)).astype(np.float32)
    sd_np[..., ::13] = 0.0
    sd_np[..., 2::31] = np.nan
    tol = 0.012
    w, sd = _cu(w_np), _cu(sd_np)
    n_votes = 0
    for name, pred_np in preds.items():
        pred = _cu(pred_np)
        for use_w in (False, True):
            for gate in (False, True):
                kw = dict(weight=w if use_w else None,
                          mesh_depth=depth if gate else None,
                          sensor_depth=sd if gate else None, depth_tol=tol if gate else None)
                votes = torch.zeros(V, NC + 1, dtype=torch.int64, device="cuda")
                assert ops.fuse_label_votes(votes, vid, pred, **kw) is votes
                ref = FN.accumulate(FN.new_table(V, NC), vid_np, pred_np,
                                    w_np if use_w else None, md_np if gate else None,
                                    sd_np if gate else None, tol if gate else None)
                case = (name, use_w, gate)
                assert np.array_equal(_u64(votes), ref), case
                assert (ref[:, 0] == 0).all()
                n_votes += int(ref.sum() > 0)
                # a second run, the uncombined form, the flat (no row structure) form
                again = torch.zeros_like(votes)
                ops.fuse_label_votes(again, vid, pred, **kw)
                assert torch.equal(again, votes), ("second run",) + case
                naive = torch.zeros_like(votes)
                ops.fuse_label_votes(naive, vid, pred, _one_atomic_per_pixel=True, **kw)
                assert torch.equal(naive, votes), ("one atomic per pixel",) + case
                flat = torch.zeros_like(votes)
                fl = lambda t: None if t is None else t.reshape(-1)  # noqa: E731
                ops.fuse_label_votes(flat, fl(vid), fl(pred), weight=fl(kw["weight"]),
                                     mesh_depth=fl(kw["mesh_depth"]),
                                     sensor_depth=fl(kw["sensor_depth"]),
                                     depth_tol=kw["depth_tol"])
                assert torch.equal(flat, votes), ("flat",) + case
                # view by view into one table
                parts = torch.zeros_like(votes)
                for b in range(shape[0]):
                    sl = lambda t: None if t is None else t[b]  # noqa: E731
                    ops.fuse_label_votes(parts, vid[b], pred[b], weight=sl(kw["weight"]),
                                         mesh_depth=sl(kw["mesh_depth"]),
                                         sensor_depth=sl(kw["sensor_depth"]),
                                         depth_tol=kw["depth_tol"])
                assert torch.equal(parts, votes), ("several calls",) + case
                for mv in (1, 50):
                    got = ops.resolve_label_votes(votes, mv)
                    label, total, winner = FN.resolve(ref, mv)
                    assert got["label"].dtype == torch.int32
                    assert np.array_equal(got["label"].cpu().numpy(), label), case
                    assert np.array_equal(_u64(got["total"]), total), case
                    assert np.array_equal(_u64(got["winner"]), winner), case
    assert n_votes == 4 * len(preds)


def test_soup_bit_exact_against_numpy():
    verts, faces, labels, rgb, poses = _soup()
    intr = (90.0, 95.0, 61.3, 47.9)
    vid, depth, clean = _ids_and_depth(verts, faces, poses, intr, 96, 128, labels)
    ref = R.rasterize(verts, faces, poses, intr, 96, 128, 0.05,
                      np.arange(1, verts.shape[0] + 1, dtype=np.int32))
    assert np.array_equal(vid.cpu().numpy(), ref["label"])
    _check_variants(verts.shape[0], vid, depth, clean, 5)


@pytest.fixture(scope="module")
def room():
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    return SyntheticRoom(0)


@pytest.mark.parametrize("step", [0.05, 1.0])
@pytest.mark.parametrize("size", [(240, 320), (480, 640)])
def test_room_bit_exact_against_numpy(room, step, size):
    H, W = size
    m = room.labelled_mesh(step)
    if step == 0.05:
        assert m["faces"].shape[0] > 180000
    else:
        assert m["faces"].shape[0] < 500
    poses, intr = room_views(H, W)
    vid, depth, clean = _ids_and_depth(m["verts"], m["faces"], poses, intr, H, W, m["labels"])
    assert (vid > 0).float().mean() > 0.99
    _check_variants(m["verts"].shape[0], vid, depth, clean, 17)


def test_a_cell_passes_two_to_the_32(room):
    ops = _ops()
    H, W = 480, 640
    m = room.labelled_mesh(1.0)
    V = m["verts"].shape[0]
    poses, intr = room_views(H, W)
    vid, _, clean = _ids_and_depth(m["verts"], m["faces"], poses, intr, H, W, m["labels"])
    w = torch.full(vid.shape, 65535, dtype=torch.int32, device="cuda")
    once = FN.accumulate(FN.new_table(V, NC), vid.cpu().numpy(), clean.cpu().numpy(),
                         w.cpu().numpy())
    # a wall corner collects ~1e5 pixels per call; at least three calls, so that
    # a cell already above 2^32 is added to again
    reps = max(3, int(2 ** 32 // int(once.max())) + 1)
    assert reps <= 64, reps
    votes = torch.zeros(V, NC + 1, dtype=torch.int64, device="cuda")
    for _ in range(reps):
        ops.fuse_label_votes(votes, vid, clean, weight=w)
    ref = once * np.uint64(reps)
    assert int(ref.max()) > 2 ** 32
    assert np.array_equal(_u64(votes), ref)
    got = ops.resolve_label_votes(votes)
    label, total, winner = FN.resolve(ref)
    assert np.array_equal(got["label"].cpu().numpy(), label)
    assert np.array_equal(_u64(got["total"]), total)
    assert np.array_equal(_u64(got["winner"]), winner)


def test_capacity_guards_and_argument_codes_through_ctypes():
    from ucsa_neural_rendering_amd import _lib
    lib = _lib.lib()
    g = np.random.default_rng(3)
    V, Cn, H, W = 50, 7, 37, 53
    N = H * W
    vid = _cu(g.integers(-1, V + 1, N).astype(np.int32))
    pred = _cu(g.integers(0, Cn + 2, N).astype(np.uint8))
    md = _cu(g.uniform(1, 2, N).astype(np.float32))
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    GUARD, MARK = 64, 0x5A5A5A5A5A5A5A5A
    cells = V * (Cn + 1)

    def table():
        t = torch.full((cells + GUARD,), MARK, dtype=torch.int64, device="cuda")
        t[:cells] = 0
        return t

    def acc(t, cap, Cn_=Cn, V_=V, N_=N, vid_=vid, pred_=pred, m=None, s=None, tol=0.0,
            flags=0):
        return lib.ucsa_label_fuse_accumulate(p(vid_), p(pred_), None, p(m), p(s), tol, N_, W,
                                              V_, Cn_, p(t), cap, flags, stream)

    t = table()
    snap = t.clone()
    assert acc(t, cells - 1) == -1011          # too small a table: nothing written
    assert acc(t, cells, Cn_=0) == -1009
    assert acc(t, cells, Cn_=256) == -1009
    assert acc(t, cells, V_=2 ** 31 // (Cn + 1) + 1) == -1008
    assert acc(t, cells, N_=2 ** 31) == -1006
    assert acc(t, cells, flags=2) == -1012
    assert acc(t, cells, m=md) == -1004        # depth without its partner
    assert acc(t, cells, s=md) == -1003
    assert acc(t, cells, m=md, s=md, tol=float("nan")) == -1005
    assert acc(t, cells, m=md, s=md, tol=-1.0) == -1005
    assert acc(t, cells, vid_=None) == -1000
    assert acc(t, cells, pred_=None) == -1001
    assert lib.ucsa_label_fuse_accumulate(p(vid), p(pred), None, None, None, 0.0, N, W, V, Cn,
                                          None, cells, 0, stream) == -1010
    # empty inputs: nothing to do, whatever the pointers
    assert acc(t, cells, N_=0, vid_=None, pred_=None) == 0
    assert acc(t, 0, V_=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(t, snap)
    assert acc(t, cells) == 0
    torch.cuda.synchronize()
    assert (t[cells:] == MARK).all()
    ref = FN.accumulate(FN.new_table(V, Cn), vid.cpu().numpy(), pred.cpu().numpy())
    assert np.array_equal(_u64(t[:cells]).reshape(V, Cn + 1), ref)

    def outs(n):
        return (torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                torch.full((n + GUARD,), MARK, dtype=torch.int64, device="cuda"),
                torch.full((n + GUARD,), MARK, dtype=torch.int64, device="cuda"))

    def res(o, cap, mv=1, V_=V, Cn_=Cn, votes=t):
        return lib.ucsa_label_fuse_resolve(p(votes), V_, Cn_, mv, p(o[0]), p(o[1]), p(o[2]), cap,
                                           stream)

    o = outs(V)
    snaps = [x.clone() for x in o]
    assert res(o, V - 1) == -1007
    assert res(o, V, mv=0) == -1003
    assert res(o, V, Cn_=0) == -1002
    assert res(o, V, votes=None) == -1000
    assert lib.ucsa_label_fuse_resolve(p(t), V, Cn, 1, None, p(o[1]), p(o[2]), V, stream) == -1004
    assert res(o, 0, V_=0, votes=None) == 0
    torch.cuda.synchronize()
    for x, y in zip(o, snaps):
        assert torch.equal(x, y)
    assert res(o, V) == 0
    torch.cuda.synchronize()
    assert (o[0][V:] == 0x5A5A5A5A).all() and (o[1][V:] == MARK).all() and (o[2][V:] == MARK).all()
    label, total, winner = FN.resolve(ref)
    assert np.array_equal(o[0][:V].cpu().numpy(), label)
    assert np.array_equal(_u64(o[1][:V]), total) and np.array_equal(_u64(o[2][:V]), winner)


def test_argument_errors_raise_and_empty_inputs():
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    votes = torch.zeros(5, NC + 1, dtype=torch.int64, device="cuda")
    vid = torch.ones(4, 6, dtype=torch.int32, device="cuda")
    pred = torch.ones(4, 6, dtype=torch.uint8, device="cuda")
    z = torch.ones(4, 6, device="cuda")
    ops.fuse_label_votes(votes, vid, pred, mesh_depth=z, sensor_depth=z, depth_tol=0.0)
    assert int(votes[0, 1]) == 24 and int(votes.sum()) == 24
    bad = [
        lambda: ops.fuse_label_votes(votes.cpu(), vid, pred),
        lambda: ops.fuse_label_votes(votes, vid.cpu(), pred),
        lambda: ops.fuse_label_votes(votes, vid, pred.cpu()),
        lambda: ops.fuse_label_votes(votes.int(), vid, pred),
        lambda: ops.fuse_label_votes(votes[:, :1], vid, pred),
        lambda: ops.fuse_label_votes(votes.view(-1), vid, pred),
        lambda: ops.fuse_label_votes(votes, vid.long(), pred),
        lambda: ops.fuse_label_votes(votes, vid, pred.int()),
        lambda: ops.fuse_label_votes(votes, vid, pred[:3]),
        lambda: ops.fuse_label_votes(votes, vid, pred, weight=vid[:2]),
        lambda: ops.fuse_label_votes(votes, vid, pred, weight=z),
        lambda: ops.fuse_label_votes(votes, vid, pred, mesh_depth=z),
        lambda: ops.fuse_label_votes(votes, vid, pred, sensor_depth=z, depth_tol=0.1),
        lambda: ops.fuse_label_votes(votes, vid, pred, mesh_depth=z, sensor_depth=z),
        lambda: ops.fuse_label_votes(votes, vid, pred, depth_tol=0.1),
        lambda: ops.fuse_label_votes(votes, vid, pred, mesh_depth=z, sensor_depth=z,
                                     depth_tol=float("nan")),
        lambda: ops.fuse_label_votes(votes, vid, pred, mesh_depth=z.half(), sensor_depth=z,
                                     depth_tol=0.1),
        lambda: ops.resolve_label_votes(votes, 0),
        lambda: ops.resolve_label_votes(votes.cpu()),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(UcsaError):
            fn()
        assert int(votes.sum()) == 24, k
    # no pixels, no vertices
    e32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    ops.fuse_label_votes(votes, e32, torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert int(votes.sum()) == 24
    none = torch.zeros(0, NC + 1, dtype=torch.int64, device="cuda")
    ops.fuse_label_votes(none, vid, pred)
    got = ops.resolve_label_votes(none)
    assert all(got[k].shape == (0,) for k in ("label", "total", "winner"))


def test_fuse_views_equals_the_cpu_pipeline():
    from ucsa_neural_rendering_amd.utils.mesh_fusion import fuse_views
    m, poses, intr, fused, held = room_setup()
    H, W = ROOM_H, ROOM_W
    ref_r = R.rasterize(m["verts"], m["faces"], poses, intr, H, W, 0.05, m["labels"])
    clean = ref_r["label"]
    noisy = noisy_labels(clean)
    ref = FN.fuse_views(m, poses[fused], intr, H, W, 0.05, noisy[fused])
    got = fuse_views(m, poses[fused], intr, H, W, 0.05, lambda i: noisy[fused[i]], batch=5)
    for k in ("labels", "total", "winner"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["observed"] == ref["observed"] and got["labels"].dtype == np.int32
    assert got["total"].dtype == np.uint64
    # the held-out comparison of the CPU test holds for the GPU path
    ops = _ops()
    rend = ops.rasterize_mesh(_cu(m["verts"]), _cu(m["faces"]), _cu(poses[held]), intr, H, W,
                              0.05, vertex_labels=_cu(got["labels"]))["label"].cpu().numpy()
    cov = clean[held] > 0
    agree = (rend[cov] == clean[held][cov]).mean()
    assert agree >= HELD_OUT_AGREE_MIN and agree > (noisy[held][cov] == clean[held][cov]).mean()
    # weights and the depth gate through the same path
    g = np.random.default_rng(9)
    wts = g.integers(0, 65536, noisy.shape).astype(np.int32)
    sd = (ref_r["depth"] + g.normal(0, 0.01, clean.shape)).astype(np.float32)
    sd[:, ::7] = 0.0
    ref = FN.fuse_views(m, poses[fused], intr, H, W, 0.05, noisy[fused], depth_maps=sd[fused],
                        depth_tol=0.012, weights=wts[fused], min_votes=3)
    got = fuse_views(m, poses[fused], intr, H, W, 0.05, noisy[fused], depth_maps=sd[fused],
                     depth_tol=0.012, weights=wts[fused], min_votes=3)
    for k in ("labels", "total", "winner"):
        assert np.array_equal(got[k], ref[k]), k
    assert 0 < got["observed"] < ref["votes"].shape[0]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


# scripts/fuse_mesh_labels.py on label_40: those maps are ray-cast (through the
# GPU's get_rays), not mesh-rendered.  Measured with the restatement pipeline on
# the CPU (8 views of _slerp_loop_poses(8, seed=123) at 240x320, the room mesh
# at step 0.1, labels from tests/test_mesh_raster_cpu.cast_room): 0 of the
# 11 670 observed vertices (share 0.4892 of 23 855) disagree with the mesh's
# own labels.  Allowed: that 0 plus 0.2 % for rays built on the GPU instead of
# in numpy (tests/test_mesh_raster_cpu.py allows 0.5 % of the pixels for it).
SCRIPT_VERTEX_DISAGREE_MAX = 0.0 + 0.002
# depth/ went through fp16 (half an ulp: z * 2^-11) and millimetre rounding: the
# bound of test_render_mesh_labels_script_end_to_end, 1 mm + z * 2^-11, at the
# largest z the room allows (its diagonal, 6 * sqrt(3) scene units = metres)
SCRIPT_DEPTH_TOL_M = (1.0 + 1000.0 * 6.0 * 3.0 ** 0.5 * 2.0 ** -11) / 1000.0


def test_fuse_mesh_labels_script_end_to_end(tmp_path, capsys):
    from PIL import Image

    from scripts import fuse_mesh_labels as script
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply, write_ply
    from ucsa_neural_rendering_amd.utils.semantic_mesh import ngp_to_pose_frame
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=8, H=240, W=320)
    m = ds.room.labelled_mesh(0.1)
    V = m["verts"].shape[0]
    rgb = np.random.default_rng(1).integers(0, 256, (V, 3)).astype(np.uint8)
    mesh = str(tmp_path / "room_geometry.ply")
    write_ply(mesh, m["verts"], m["faces"], rgb=rgb)  # no labels in the input
    out = str(tmp_path / "fused" / "room.labels.ply")
    rec = script.main(["--scene_root", sroot, "--mesh", mesh, "--labels", "label_40", "--out",
                       out])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == rec["frames"] == 8 and line["vertices"] == V
    assert set(line["fuse_ms_per_view"]) == {"rasterize", "accumulate"}
    f = read_ply(out)
    assert np.array_equal(f["verts"], m["verts"]) and np.array_equal(f["faces"], m["faces"])
    assert np.array_equal(f["rgb"], rgb)  # the input's colours, none invented
    labels = f["labels"]
    obs = labels > 0
    assert obs.sum() == rec["observed"] > 0.4 * V
    disagree = (labels[obs] != m["labels"][obs]).mean()
    with capsys.disabled():
        print(f"\nlabel_40 -> mesh: observed {obs.mean():.4f}, vertex disagreement "
              f"{disagree:.5f}")
    assert disagree <= SCRIPT_VERTEX_DISAGREE_MAX
    # the mesh in the JSON pose frame, in metres: the same labels, written back
    # in that frame
    mesh_pf = str(tmp_path / "room_pose_frame.ply")
    verts_pf = ngp_to_pose_frame(m["verts"], ds.one_m_to_scene_uom)
    write_ply(mesh_pf, verts_pf, m["faces"])
    out_pf = str(tmp_path / "room_pf.labels.ply")
    script.main(["--scene_root", sroot, "--mesh", mesh_pf, "--pose_frame", "--labels",
                 os.path.join(sroot, "label_40"), "--out", out_pf])
    fp = read_ply(out_pf)
    assert np.array_equal(fp["labels"], labels) and "rgb" not in fp
    assert np.array_equal(fp["verts"], np.asarray(verts_pf, np.float32))
    # the depth gate with the scene's own depth/ keeps the result ...
    out_d = str(tmp_path / "room_depth.labels.ply")
    script.main(["--scene_root", sroot, "--mesh", mesh, "--labels", "label_40", "--depth_tol",
                 repr(SCRIPT_DEPTH_TOL_M), "--out", out_d])
    assert np.array_equal(read_ply(out_d)["labels"], labels)
    # ... and with depth maps a metre off nothing votes
    far = tmp_path / "far"
    os.makedirs(far / "depth")
    for name in ("transforms_train.json",):
        os.symlink(os.path.join(sroot, name), far / name)
    os.symlink(os.path.join(sroot, "label_40"), far / "label_40")
    for s in sorted(os.listdir(os.path.join(sroot, "depth"))):
        d = _png(os.path.join(sroot, "depth", s)).astype(np.int64) + 1000
        Image.fromarray(np.clip(d, 0, 65535).astype(np.uint16)).save(str(far / "depth" / s))
    out_far = str(tmp_path / "room_far.labels.ply")
    rec_far = script.main(["--scene_root", str(far), "--mesh", mesh, "--labels", "label_40",
                           "--depth_tol", repr(SCRIPT_DEPTH_TOL_M), "--out", out_far])
    assert rec_far["observed"] == 0 and (read_ply(out_far)["labels"] == 0).all()
    # noisy frame predictions: the fused map scores above its input
    exp = os.path.join(sroot, "exp")
    os.makedirs(os.path.join(exp, "seg_label"))
    g = np.random.default_rng(7)
    for s in sorted(os.listdir(os.path.join(sroot, "label_40"))):
        lab = _png(os.path.join(sroot, "label_40", s))
        flip = g.random(lab.shape) < 0.4
        noisy = lab.copy()
        noisy[flip] = g.integers(1, 41, int(flip.sum()))
        Image.fromarray(noisy.astype(np.uint8)).save(os.path.join(exp, "seg_label", s))
    capsys.readouterr()
    script.main(["--scene_root", sroot, "--mesh", mesh, "--labels", "seg_label", "--exp_name",
                 "exp", "--every", "2", "--out", str(tmp_path / "seg.labels.ply"), "--render",
                 "--score"])
    text = capsys.readouterr().out.strip().splitlines()[-1]
    line = json.loads(text)
    with capsys.disabled():
        print(text)
    assert line["frames"] == 4
    assert _png(os.path.join(exp, "map_label", "000002.png")).dtype == np.uint8
    assert not os.path.exists(os.path.join(exp, "map_label", "000001.png"))
    assert line["fused"]["mIoU"] > line["input"]["mIoU"]
    assert line["fused"]["total_acc"] > line["input"]["total_acc"]
