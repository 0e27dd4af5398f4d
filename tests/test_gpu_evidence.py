"""GPU: soft label fusion (k_tsdf_evidence / k_evidence_resolve of
csrc/voxel_map.hip, k_lf_evidence of csrc/label_fusion.hip) against the numpy
restatement of its contracts (tests/evidence_numpy.py), bit for bit; the hand
case of tests/test_evidence_cpu.py through the ops; both scripts with --scores
on an exported synthetic scene."""
import json
import os

import numpy as np
import pytest
import torch

from tests import evidence_numpy as EN
from tests import fusion_numpy as FN
from tests import tsdf_numpy as TN
from tests.test_evidence_cpu import HAND_ROWS, hand_voxel_case
from tests.test_gpu_tsdf_fusion import _cu, _ops, guarded_volume
from tests.test_gpu_voxel_map import guarded
from tests.test_tsdf_fusion_cpu import look_at

pytestmark = pytest.mark.gpu

F32 = np.float32
DIMS, H, W, B = (19, 10, 33), 24, 32, 5
INTR = (30.0, 28.5, 15.65, 12.3)
SENTINEL = 0xDEAD0000


def voxel_case(seed=0):
    """An odd lattice with anisotropic spacing (19*10*33 = 6270 voxels: partial
    waves, bricks and work-groups), five cameras around it, views 1 and 3
    looking away from it, depth with every kind of invalid value."""
    g = np.random.default_rng(seed)
    origin = np.array([-0.4, 0.3, -0.9], F32)
    spacing = np.array([0.05, 0.06, 0.055], F32)
    ext = (np.array(DIMS) - 1) * spacing.astype(np.float64)
    centre = origin + ext / 2
    poses, depth = [], []
    for b in range(B):
        d = g.normal(size=3)
        d /= np.linalg.norm(d)
        eye = centre + d * g.uniform(2.5, 3.5)
        target = centre + g.uniform(-0.2, 0.2, 3) * ext
        if b in (1, 3):
            target = eye + (eye - centre)
        poses.append(look_at(eye, target, up=g.normal(size=3)))
        ys, xs = np.mgrid[0:H, 0:W]
        z = np.linalg.norm(eye - centre) + 0.5 * np.sin(xs / 5.0 + b) * np.cos(ys / 4.0 - b)
        z = z.astype(F32)
        z[g.random(z.shape) < 0.03] = 0.0
        z[g.random(z.shape) < 0.02] = np.nan
        z[g.random(z.shape) < 0.02] = np.inf
        z[g.random(z.shape) < 0.02] *= -1.0
        z[g.random(z.shape) < 0.02] = 9.0
        depth.append(z)
    return {"dims": DIMS, "origin": origin, "spacing": spacing, "poses": np.stack(poses),
            "depth": np.stack(depth), "intr": INTR, "trunc": 0.3, "depth_min": 0.05,
            "depth_max": 8.0}


def random_scores(seed, shape, C):
    """codes with every tenth row all zero and, for C > 40, rows whose only
    non-zero code lies past class 40"""
    g = np.random.default_rng(seed)
    s = g.integers(0, 256, shape + (C,)).astype(np.uint8)
    kind = g.integers(0, 10, shape)
    s[kind == 0] = 0
    if C > 40:
        late = kind == 1
        s[late] = 0
        s[late, C - 3] = 7
    return s


@pytest.fixture(scope="module")
def case():
    c = voxel_case()
    c["vol"] = TN.new_volume(c["dims"], c["origin"], c["spacing"])
    c["want"], c["reached"] = {}, np.zeros(DIMS, bool)
    for C in (1, 5, 40, 255):
        sc = random_scores(C, (B, H, W), C)
        ev = EN.new_evidence(DIMS, C)
        ev[:] = SENTINEL
        EN.accumulate(ev, c["vol"], c["depth"], sc, c["poses"], INTR, c["trunc"], c["depth_min"],
                      c["depth_max"], reached=c["reached"])
        c["want"][C] = (sc, ev)
    return c


def run_gpu(c, scores, order, splits, fill=SENTINEL):
    ops = _ops()
    C = scores.shape[-1]
    vol, vcheck = guarded_volume(c["dims"], c["origin"], c["spacing"], False)
    ev, check = guarded((C + 1,) + tuple(c["dims"]), torch.uint32, 0)
    ev.view(torch.int32).fill_(int(np.uint32(fill).view(np.int32)))
    # the rows start at an odd address: one byte into a buffer
    raw = torch.zeros(scores.size + 1, dtype=torch.uint8, device="cuda")
    raw[1:] = _cu(scores.reshape(-1))
    sc = raw[1:].view(scores.shape)
    assert sc.data_ptr() % 4 == 1
    depth, poses = _cu(c["depth"]), _cu(c["poses"])
    for a, b in splits:
        s = list(order[a:b])
        if s == list(range(s[0], s[0] + len(s))):
            s = slice(s[0], s[0] + len(s))      # a slice: the rows keep their odd address
        else:
            s = torch.as_tensor(s, device="cuda")
        ops.accumulate_voxel_evidence(ev, vol, depth[s], sc[s], poses[s], c["intr"], c["trunc"],
                                      depth_min=c["depth_min"], depth_max=c["depth_max"])
    torch.cuda.synchronize()
    check()
    vcheck()
    return ev


@pytest.mark.parametrize("C", [1, 5, 40, 255])
def test_voxel_evidence_bit_exact_for_every_split_and_order(case, C):
    scores, want = case["want"][C]
    reached = case["reached"]
    assert 0.1 < reached.mean() < 0.9
    took = want[0] != SENTINEL
    assert took.sum() > 300 and (reached & ~took).sum() > 10      # all-zero rows abstained
    assert (want[0][took] - np.uint32(SENTINEL)).max() >= 2       # voxels with several views
    for order, splits in ((range(B), [(0, B)]), (range(B), [(i, i + 1) for i in range(B)]),
                          (range(B - 1, -1, -1), [(0, B)]), ([2, 0, 4, 3, 1], [(0, 2), (2, B)])):
        got = run_gpu(case, scores, list(order), splits).cpu().numpy()
        assert got.tobytes() == want.tobytes(), (C, list(order), splits)
    # a voxel that no view reaches in its band keeps the poison in every plane
    assert (got[:, ~reached] == SENTINEL).all()


def test_voxel_evidence_saturates_in_every_plane():
    ops = _ops()
    vol_np, depth, poses, intr, trunc, scores, band = hand_voxel_case()
    scores[:] = 255
    vol = ops.tsdf_volume((2, 2, 9), vol_np["origin"], 0.1)
    for splits in ([(0, 3)], [(0, 1), (1, 2), (2, 3)]):
        ev = ops.voxel_evidence(vol, 2)
        ev.view(torch.int32).fill_(-3)                            # 2^32 - 3
        for a, b in splits:
            ops.accumulate_voxel_evidence(ev, vol, _cu(depth[a:b]), _cu(scores[a:b]),
                                          _cu(poses[a:b]), intr, trunc)
        got = ev.cpu().numpy()
        assert (got[:, :, :, band] == EN.SAT).all() and (got[:, :, :, ~band] == EN.SAT - 2).all()


def test_resolve_bit_exact_ties_gates_and_one_class():
    ops = _ops()
    g = np.random.default_rng(5)
    for C in (1, 2, 7, 40):
        ev = g.integers(0, 6, (C + 1, 7, 5, 13)).astype(np.uint32)   # small values: many ties
        ev[:, 0, 0, :4] = g.integers(2 ** 31, 2 ** 32, (C + 1, 4))   # the top bit
        ev[1:, 1, 1, 1] = 9                                          # every class ties: 1
        for mv, mm in ((1, 0), (3, 0), (1, 2), (2, 1), (1, 2 ** 32 - 1)):
            got = ops.resolve_voxel_evidence(_cu(ev), mv, mm)
            want = EN.resolve(ev, mv, mm)
            for k, w in zip(("label", "views", "best", "margin"), want):
                x = got[k].cpu().numpy()
                assert x.dtype == w.dtype and x.tobytes() == w.tobytes(), (C, mv, mm, k)
        lab = EN.resolve(ev)[0]
        assert lab[1, 1, 1] == 1 and EN.resolve(ev)[3][1, 1, 1] == (9 if C == 1 else 0)
    from ucsa_neural_rendering_amd._lib import UcsaError
    with pytest.raises(UcsaError):
        ops.resolve_voxel_evidence(_cu(ev), 0)
    with pytest.raises(UcsaError):
        ops.resolve_voxel_evidence(_cu(ev).view(torch.int32))


N_PIX, V = 64 * 3 + 17, 50


def mesh_case(C, seed=3):
    g = np.random.default_rng(seed)
    vid = g.integers(1, V + 1, N_PIX).astype(np.int32)
    vid[0:64] = 7                                             # a whole wave on one vertex
    vid[64:114] = g.permutation(V) + 1                        # every lane another vertex
    vid[114:128] = [0, -1, V + 1, 1000, -2 ** 31, 2 ** 31 - 1, 0, -5, V + 7, 0, 51, -1, 0, 99]
    vid[120:140] = 9                                          # a run across a wave boundary
    vid[200:] = 33
    scores = random_scores(seed + 1, (N_PIX,), C)
    mesh_z = g.uniform(1.0, 2.0, N_PIX).astype(F32)
    sensor_z = (mesh_z + g.normal(0, 0.02, N_PIX)).astype(F32)
    sensor_z[g.random(N_PIX) < 0.1] = 0.0
    sensor_z[g.random(N_PIX) < 0.05] = np.nan
    mesh_z[g.random(N_PIX) < 0.05] = np.nan
    return vid, scores, mesh_z, sensor_z


@pytest.mark.parametrize("C", [1, 40])
def test_mesh_evidence_bit_exact(C):
    ops = _ops()
    vid, scores, mesh_z, sensor_z = mesh_case(C)
    tol = 0.02
    for gate in (False, True):
        kw_np = dict(mesh_depth=mesh_z, sensor_depth=sensor_z, depth_tol=tol) if gate else {}
        want = EN.fuse(FN.new_table(V, C), vid, scores, **kw_np)
        assert (want[:, 0] == 0).all() and want[6, 1:].sum() > 64 * (0 if gate else 20)
        # flat (one 16x16 tile holds it all), as rows of 19 (two tiles side by side, the
        # second three pixels wide) and of 11, and in two calls
        for shape, cuts in (((N_PIX,), [(0, N_PIX)]), ((11, 19), [(0, 11)]), ((19, 11), [(0, 19)]),
                            ((N_PIX,), [(0, 100), (100, N_PIX)]), ((19, 11), [(7, 19), (0, 7)])):
            table, check = guarded((V, C + 1), torch.int64, 0)
            v2, s2 = vid.reshape(shape), scores.reshape(shape + (C,))
            m2, z2 = mesh_z.reshape(shape), sensor_z.reshape(shape)
            for a, b in cuts:
                kw = dict(mesh_depth=_cu(m2[a:b]), sensor_depth=_cu(z2[a:b]),
                          depth_tol=tol) if gate else {}
                assert ops.fuse_label_evidence(table, _cu(v2[a:b]), _cu(s2[a:b]), **kw) is table
            torch.cuda.synchronize()
            check()
            got = table.cpu().numpy().view(np.uint64)
            assert got.tobytes() == want.tobytes(), (C, gate, shape, cuts)
        assert (got[:, 0] == 0).all()
        for mv in (1, 300):
            res = ops.resolve_label_votes(table, mv)
            for k, w in zip(("label", "total", "winner"), FN.resolve(want, mv)):
                x = res[k].cpu().numpy()
                assert x.view(w.dtype).tobytes() == w.tobytes(), (C, gate, mv, k)
    from ucsa_neural_rendering_amd._lib import UcsaError
    with pytest.raises(UcsaError):
        ops.fuse_label_evidence(table, _cu(vid), _cu(scores[:, :1].repeat(C + 1, 1)))
    with pytest.raises(UcsaError):
        ops.fuse_label_evidence(table, _cu(vid), _cu(scores), mesh_depth=_cu(mesh_z))


def test_hand_case_on_the_device_for_both_routes():
    ops = _ops()
    vol_np, depth, poses, intr, trunc, scores, band = hand_voxel_case()
    vol = ops.tsdf_volume((2, 2, 9), vol_np["origin"], 0.1)
    ev = ops.accumulate_voxel_evidence(ops.voxel_evidence(vol, 2), vol, _cu(depth), _cu(scores),
                                       _cu(poses), intr, trunc)
    got = ev.cpu().numpy()
    assert (got[0][:, :, band] == 3).all() and (got[1][:, :, band] == 617).all()
    assert (got[2][:, :, band] == 696).all() and not got[:, :, :, ~band].any()
    res = ops.resolve_voxel_evidence(ev)
    assert (res["label"].cpu().numpy()[:, :, band] == 2).all()
    assert (res["margin"].cpu().numpy()[:, :, band] == 79).all()
    assert not ops.resolve_voxel_evidence(ev, min_margin=80)["label"].any()
    assert (ops.resolve_voxel_evidence(ev, min_margin=79)["label"].cpu().numpy()[:, :, band]
            == 2).all()
    pred = _cu((scores.argmax(-1) + 1).astype(np.uint8))
    votes = ops.vote_voxel_labels(ops.voxel_votes(vol, 2), vol, _cu(depth), pred, _cu(poses),
                                  intr, trunc)
    assert (ops.resolve_voxel_labels(votes)["label"].cpu().numpy()[:, :, band] == 1).all()
    # one vertex, three pixels
    vid = _cu(np.array([4, 4, 4], np.int32))
    table = ops.fuse_label_evidence(torch.zeros(6, 3, dtype=torch.int64, device="cuda"), vid,
                                    _cu(HAND_ROWS))
    assert table[3].tolist() == [0, 617, 696] and int(table.sum()) == 617 + 696
    assert ops.resolve_label_votes(table)["label"].tolist() == [0, 0, 0, 2, 0, 0]
    hard = ops.fuse_label_votes(torch.zeros(6, 3, dtype=torch.int64, device="cuda"), vid,
                                _cu((HAND_ROWS.argmax(1) + 1).astype(np.uint8)))
    assert ops.resolve_label_votes(hard)["label"].tolist() == [0, 0, 0, 1, 0, 0]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_scripts_with_scores_reproduce_the_hard_route_on_confident_beliefs(tmp_path, capsys):
    from scripts import fuse_mesh_labels, voxel_map_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply, write_ply
    ops = _ops()
    Hs, Ws, n, C = 240, 320, 8, 40
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=Hs, W=Ws)
    # beliefs from label_40: 0.9 on the true class, the rest spread evenly; a
    # pixel without a label abstains
    os.makedirs(tmp_path / "codes")
    for b in range(n):
        stem = f"{b:06d}"
        lab = torch.from_numpy(_png(os.path.join(sroot, "label_40", stem + ".png")).astype(
            np.int64)).cuda()
        p = torch.full((1, C, Hs, Ws), 0.1 / (C - 1), device="cuda")
        p.scatter_(1, (lab.clamp(min=1) - 1)[None, None], 0.9)
        codes = ops.log_evidence(p)[0]
        codes[lab == 0] = 0
        codes = codes.cpu().numpy()
        assert codes.shape == (Hs, Ws, C) and set(np.unique(codes)) <= {0, 65, 252}
        np.save(tmp_path / "codes" / (stem + ".npy"),
                codes if b % 2 else np.ascontiguousarray(codes.transpose(2, 0, 1)))
    h = 6.1 / 63
    common = ["--scene_root", sroot, "--voxel", repr(h), "--step", repr(0.5 * h), "--aabb",
              "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05", "--score"]
    capsys.readouterr()
    hard = voxel_map_labels.main(common + ["--labels", "label_40", "--out_dir",
                                           str(tmp_path / "hard")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # without --scores the record is what it was
    assert sorted(line) == ["dims", "frames", "fuse_ms_per_view", "input", "labelled", "labels",
                            "observed", "out_dir", "raycast_ms_per_view", "voxel_map"]
    soft = voxel_map_labels.main(common + ["--scores", str(tmp_path / "codes"), "--out_dir",
                                           str(tmp_path / "soft")])
    assert soft["scores"] == str(tmp_path / "codes") and soft["dims"] == hard["dims"] == [64] * 3
    assert soft["labelled"] == hard["labelled"] > 0.05
    assert soft["voxel_map"] == hard["voxel_map"] and soft["input"]["mIoU"] > 0.999
    for b in range(n):
        stem = f"{b:06d}.png"
        for k in ("map_label", "map_depth"):
            assert _png(tmp_path / "soft" / k / stem).tobytes() == \
                _png(tmp_path / "hard" / k / stem).tobytes(), (k, b)
    assert (_png(tmp_path / "soft" / "map_label" / "000000.png") > 0).mean() > 0.3
    # a margin no voxel reaches: nothing is labelled; --labels names the scored input
    none = voxel_map_labels.main(common + ["--scores", str(tmp_path / "codes"), "--labels",
                                           "label_40", "--min_margin", str(255 * n + 1),
                                           "--out_dir", str(tmp_path / "none")])
    assert none["labelled"] == 0.0 and none["input"] == hard["input"]
    with pytest.raises(SystemExit):
        voxel_map_labels.main(common + ["--out_dir", str(tmp_path / "x")])
    with pytest.raises(SystemExit):
        voxel_map_labels.main(common + ["--labels", "label_40", "--min_margin", "2", "--out_dir",
                                        str(tmp_path / "x")])
    # the mesh route
    m = ds.room.labelled_mesh(0.1)
    mesh = str(tmp_path / "room_geometry.ply")
    write_ply(mesh, m["verts"], m["faces"])
    args = ["--scene_root", sroot, "--mesh", mesh]
    capsys.readouterr()
    rh = fuse_mesh_labels.main(args + ["--labels", "label_40", "--out", str(tmp_path / "h.ply")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(line) == ["faces", "frames", "fuse_ms_per_view", "labels", "observed", "out",
                            "vertices"]
    rs = fuse_mesh_labels.main(args + ["--scores", str(tmp_path / "codes"), "--out",
                                       str(tmp_path / "s.ply")])
    lh, ls = read_ply(str(tmp_path / "h.ply"))["labels"], read_ply(str(tmp_path / "s.ply"))["labels"]
    assert rs["observed"] == rh["observed"] > 0.3 * m["verts"].shape[0]
    assert np.array_equal(ls, lh)
    rg = fuse_mesh_labels.main(args + ["--scores", str(tmp_path / "codes"), "--depth_tol", "0.05",
                                       "--min_margin", "188", "--out", str(tmp_path / "g.ply")])
    lg = read_ply(str(tmp_path / "g.ply"))["labels"]
    assert 0 < rg["observed"] <= rs["observed"] and ((lg == 0) | (lg == ls)).all()
