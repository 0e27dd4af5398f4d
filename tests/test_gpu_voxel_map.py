"""GPU: the voxel map (csrc/voxel_map.hip) against the numpy restatement of its
contracts (tests/voxel_map_numpy.py), bit for bit: votes and resolve for every
batch size, ray-cast with and without colour, labels and empty-space skipping;
guard words, argument codes; the room's depth, coverage and mIoU conditions of
tests/test_voxel_map_cpu.py on the device; scripts/voxel_map_labels.py end to
end from a scene directory."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import tsdf_numpy as TN
from tests import voxel_map_numpy as VN
from tests.test_gpu_tsdf_fusion import _cu, _ops, guarded_volume
from tests.test_tsdf_fusion_cpu import batches, room_volume_spec
from tests.test_voxel_map_cpu import (COVER_MIN, DISAGREE_MAX, ROOM_ACC, ROOM_FAR, ROOM_MIOU,
                                      ROOM_NEAR, build_room, check_room_depth,
                                      random_raycast_case, random_vote_case, room_raycast, score)

pytestmark = pytest.mark.gpu

GUARD = 1024  # elements before and after each buffer
# 0.02 under the figures measured with the restatement (tests/test_voxel_map_cpu.py)
MIOU_MIN, ACC_MIN = ROOM_MIOU - 0.02, ROOM_ACC - 0.02


def guarded(shape, dtype, fill):
    """a tensor that is a view into a larger buffer of a guard pattern -> (t, check())"""
    n = int(np.prod(shape))
    store = torch.int16 if dtype == torch.uint16 else (torch.int32 if dtype == torch.uint32
                                                       else dtype)
    pat = 77 if store == torch.uint8 else -777
    b = torch.full((2 * GUARD + n,), pat, dtype=store, device="cuda")
    b[GUARD:GUARD + n] = fill
    t = b[GUARD:GUARD + n].view(dtype).view(shape)

    def check():
        assert (b[:GUARD] == pat).all() and (b[-GUARD:] == pat).all()
    return t, check


def vol_to_gpu(vol):
    return {"tsdf": _cu(vol["tsdf"]), "weight": _cu(vol["weight"]),
            "rgb": None if vol["rgb"] is None else _cu(vol["rgb"]),
            "origin": tuple(float(v) for v in vol["origin"]),
            "spacing": tuple(float(v) for v in vol["spacing"])}


def vote_gpu(case, splits, n_classes=40):
    ops = _ops()
    vol, _ = guarded_volume(case["dims"], case["origin"], case["spacing"], False)
    votes, check = guarded((n_classes + 1,) + tuple(case["dims"]), torch.uint16, 0)
    depth, poses, pred = _cu(case["depth"]), _cu(case["poses"]), _cu(case["pred"])
    for a, b in splits:
        ops.vote_voxel_labels(votes, vol, depth[a:b], pred[a:b], poses[a:b], case["intr"],
                              case["trunc"], depth_min=case["depth_min"],
                              depth_max=case["depth_max"])
    torch.cuda.synchronize()
    check()
    return votes


def vote_numpy(case, n_classes=40):
    vol = TN.new_volume(case["dims"], case["origin"], case["spacing"])
    return VN.vote(VN.new_votes(case["dims"], n_classes), vol, case["depth"], case["pred"],
                   case["poses"], case["intr"], case["trunc"], case["depth_min"],
                   case["depth_max"])


def check_resolve(votes_gpu, votes_np, min_votes):
    got = _ops().resolve_voxel_labels(votes_gpu, min_votes)
    want = VN.resolve(votes_np, min_votes)
    for k, w in zip(("label", "total", "winner"), want):
        g = got[k].cpu().numpy()
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (k, min_votes)


def test_votes_and_resolve_bit_exact_for_every_batch_size_and_twice():
    case = random_vote_case(0, 16)
    want = vote_numpy(case)
    assert (want[1:].sum(0) > 0).mean() > 0.2 and want.max() >= 2
    for size in (1, 5, 16, 16):
        got = vote_gpu(case, batches(16, size))
        assert got.cpu().numpy().tobytes() == want.tobytes(), size
    for mv in (1, 2):
        check_resolve(got, want, mv)
    few = vote_gpu(case, [(0, 16)], n_classes=20)   # classes above C do not vote
    assert few.cpu().numpy().tobytes() == want[:21].tobytes()


def test_more_views_than_one_launch_takes():
    case = random_vote_case(3, 40)  # 32 views per launch: two launches in one call
    want = vote_numpy(case)
    assert vote_gpu(case, [(0, 40)]).cpu().numpy().tobytes() == want.tobytes()
    assert vote_gpu(case, [(0, 33), (33, 40)]).cpu().numpy().tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def room_case():
    rc = build_room(240, 320, 128)
    rc["case"] = {"dims": rc["dims"], "origin": np.asarray(rc["vol"]["origin"], np.float32),
                  "spacing": rc["vol"]["spacing"], "poses": rc["poses"], "depth": rc["depth"],
                  "pred": rc["pred"], "intr": rc["intr"], "trunc": rc["trunc"],
                  "depth_min": 1e-6, "depth_max": 3.0e38}
    return rc


def test_room_votes_bit_exact_for_every_batch_size_and_twice(room_case):
    rc = room_case
    for size in (1, 5, 16, 16):
        got = vote_gpu(rc["case"], batches(16, size))
        assert got.cpu().numpy().tobytes() == rc["votes"].tobytes(), size
    check_resolve(got, rc["votes"], 1)
    check_resolve(got, rc["votes"], 3)


def raycast_gpu(vol, args, labels, plain, step=None):
    """ops.raycast_tsdf into guarded outputs is not possible (it allocates), so the
    C entry is driven directly with the same arguments -> dict of numpy arrays"""
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    poses, intr, H, W, near, far, trunc = args
    B = poses.shape[0]
    step = 0.5 * trunc if step is None else step
    g = vol_to_gpu(vol)
    nx, ny, nz = vol["tsdf"].shape
    outs, checks = {}, []
    spec = [("depth", (B, H, W), torch.float32), ("voxel_id", (B, H, W), torch.int32),
            ("normal", (B, H, W, 3), torch.float32)]
    if g["rgb"] is not None:
        spec.append(("rgb", (B, H, W, 3), torch.float32))
    if labels is not None:
        spec.append(("label", (B, H, W), torch.int32))
    for k, shape, dt in spec:
        outs[k], c = guarded(shape, dt, 5)
        checks.append(c)
    nb = int(l.ucsa_tsdf_raycast_workspace_bytes(nx, ny, nz))
    ws, c = guarded((nb,), torch.uint8, 9)
    checks.append(c)
    lab = None if labels is None else _cu(labels)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = l.ucsa_tsdf_raycast(
        p(g["tsdf"]), p(g["weight"]), p(g["rgb"]), p(lab), nx, ny, nz, _lib.fvec(g["origin"]),
        _lib.fvec(g["spacing"]), p(_cu(poses)), B, *[float(v) for v in intr], H, W, near, far,
        float(trunc), float(step), 1.0, p(outs["depth"]), p(outs["voxel_id"]), p(outs["normal"]),
        p(outs.get("rgb")), p(outs.get("label")), B * H * W, None if plain else p(ws),
        0 if plain else nb, 1 if plain else 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    for c in checks:
        c()
    return {k: v.cpu().numpy() for k, v in outs.items()}


def assert_same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k)


def test_raycast_random_case_bit_exact_with_and_without_colour_labels_and_skipping():
    ops = _ops()
    vol, lab, args = random_raycast_case(0)
    want = VN.raycast(vol, *args, voxel_labels=lab)
    assert 0.2 < (want["voxel_id"] >= 0).mean() < 0.9
    for plain in (False, True):
        assert_same(raycast_gpu(vol, args, lab, plain), want, plain)
    bare = dict(vol, rgb=None)
    want_bare = {k: want[k] for k in ("depth", "voxel_id", "normal")}
    for plain in (False, True):
        assert_same(raycast_gpu(bare, args, None, plain), want_bare, plain)
    assert_same(raycast_gpu(vol, args, None, False), {k: want[k] for k in want if k != "label"},
                "colour, no labels")
    # B = 1, through ops, with a step of its own
    one = (args[0][5:6],) + args[1:]
    want1 = VN.raycast(vol, *one, step=0.07, voxel_labels=lab)
    for plain in (False, True):
        got = ops.raycast_tsdf(vol_to_gpu(vol), _cu(one[0]), *one[1:6], step=0.07,
                               voxel_labels=_cu(lab), trunc=one[6], _plain_march=plain)
        assert_same({k: v.cpu().numpy() for k, v in got.items()}, want1, ("ops", plain))


def test_room_raycast_bit_exact_and_within_the_bounds(room_case, capsys):
    rc = room_case
    want = room_raycast(rc)
    args = (rc["poses"], rc["intr"], rc["H"], rc["W"], ROOM_NEAR, ROOM_FAR, rc["trunc"])
    for plain in (False, True, False):   # skipping, plain, twice
        assert_same(raycast_gpu(rc["vol"], args, rc["label"], plain, step=rc["step"]), want, plain)
    # the whole route on the device: integrate + vote in batches, resolve, ray-cast
    ops = _ops()
    vol = ops.tsdf_volume(rc["dims"], rc["vol"]["origin"], rc["h"])
    votes = ops.voxel_votes(vol, 40)
    depth, poses, pred = _cu(rc["depth"]), _cu(rc["poses"]), _cu(rc["pred"])
    for a, b in batches(16, 5):
        ops.integrate_tsdf(vol, depth[a:b], poses[a:b], rc["intr"], rc["trunc"])
        ops.vote_voxel_labels(votes, vol, depth[a:b], pred[a:b], poses[a:b], rc["intr"],
                              rc["trunc"])
    labels = ops.resolve_voxel_labels(votes)["label"]
    assert labels.cpu().numpy().tobytes() == rc["label"].tobytes()
    out = ops.raycast_tsdf(vol, poses, rc["intr"], rc["H"], rc["W"], ROOM_NEAR, ROOM_FAR,
                           step=rc["step"], voxel_labels=labels, trunc=rc["trunc"])
    assert_same({k: v.cpu().numpy() for k, v in out.items()}, want, "device route")
    with capsys.disabled():
        print()
        check_room_depth(out["depth"].cpu().numpy(), rc)
        s = score(out["label"].cpu().numpy(), rc["pred"])
        print(f"voxel map on the device: mIoU {s['mIoU']:.4f}, accuracy {s['total_acc']:.4f}")
    assert s["mIoU"] >= MIOU_MIN and s["total_acc"] >= ACC_MIN


def test_argument_codes_come_before_any_launch():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dims = (8, 9, 10)
    n = 8 * 9 * 10
    vol, vcheck = guarded_volume(dims, (0, 0, 0), 0.1, True)
    vol["weight"].fill_(1.0)
    vol["tsdf"][:, :, 5:] = -1.0
    votes, check = guarded((6,) + dims, torch.uint16, 0)
    depth = torch.ones(2, 12, 16, device="cuda")
    pred = torch.full((2, 12, 16), 2, dtype=torch.uint8, device="cuda")
    poses = torch.eye(4, device="cuda").repeat(2, 1, 1).contiguous()
    o, h = _lib.fvec((0, 0, 0)), _lib.fvec((0.1, 0.1, 0.1))
    base = dict(votes=p(votes), cap=6 * n, C=5, nx=8, ny=9, nz=10, origin=o, spacing=h,
                depth=p(depth), pred=p(pred), poses=p(poses), B=2, fx=10.0, fy=10.0, cx=8.0,
                cy=6.0, H=12, W=16, trunc=0.3, dmin=0.01, dmax=5.0, stream=None)

    def rc(**kw):
        return l.ucsa_tsdf_vote(*{**base, **kw}.values())
    for kw, code in ((dict(votes=None), 0), (dict(cap=6 * n - 1), 1), (dict(C=0), 2),
                     (dict(C=256), 2), (dict(nx=1), 3), (dict(ny=1), 4), (dict(nz=1), 5),
                     (dict(origin=None), 6), (dict(spacing=None), 7), (dict(depth=None), 8),
                     (dict(pred=None), 9), (dict(poses=None), 10), (dict(B=0), 11),
                     (dict(fx=0.0), 12), (dict(fy=-1.0), 13), (dict(H=0), 16),
                     (dict(W=16385), 17), (dict(trunc=0.0), 18),
                     (dict(dmin=float("nan")), 19), (dict(dmax=0.001), 20)):
        assert rc(**kw) == -1000 - code, (kw, code)
    torch.cuda.synchronize()
    check()
    assert not votes.cpu().numpy().any()   # an argument error launches nothing
    assert rc() == 0
    torch.cuda.synchronize()
    check()
    assert votes[2].cpu().numpy().any() and not votes[0].cpu().numpy().any()
    # resolve
    lab, c1 = guarded(dims, torch.uint8, 9)
    tot, c2 = guarded(dims, torch.uint32, 9)
    win, c3 = guarded(dims, torch.uint32, 9)
    res = lambda *a: l.ucsa_voxel_label_resolve(*a)
    assert res(None, 5, n, 1, p(lab), p(tot), p(win), n, None) == -1000
    assert res(p(votes), 0, n, 1, p(lab), p(tot), p(win), n, None) == -1001
    assert res(p(votes), 256, n, 1, p(lab), p(tot), p(win), n, None) == -1001
    assert res(p(votes), 5, n, 0, p(lab), p(tot), p(win), n, None) == -1003
    assert res(p(votes), 5, n, 1, p(lab), p(tot), p(win), n - 1, None) == -1007
    torch.cuda.synchronize()
    assert (lab == 9).all() and (tot.cpu().numpy() == 9).all()
    assert res(p(votes), 5, n, 1, p(lab), p(tot), p(win), n, None) == 0
    torch.cuda.synchronize()
    for c in (c1, c2, c3):
        c()
    assert set(np.unique(lab.cpu().numpy())) <= {0, 2}
    # ray-cast
    nb = int(l.ucsa_tsdf_raycast_workspace_bytes(*dims))
    assert nb >= 4 and l.ucsa_tsdf_raycast_workspace_bytes(1, 9, 10) == 0
    outs = {k: guarded(s, d, 5) for k, s, d in (("depth", (2, 12, 16), torch.float32),
                                                ("vid", (2, 12, 16), torch.int32),
                                                ("normal", (2, 12, 16, 3), torch.float32),
                                                ("rgb", (2, 12, 16, 3), torch.float32),
                                                ("label", (2, 12, 16), torch.int32))}
    ws, wcheck = guarded((nb,), torch.uint8, 9)
    rbase = dict(tsdf=p(vol["tsdf"]), weight=p(vol["weight"]), rgb=p(vol["rgb"]), labels=p(lab),
                 nx=8, ny=9, nz=10, origin=o, spacing=h, poses=p(poses), B=2, fx=10.0, fy=10.0,
                 cx=8.0, cy=6.0, H=12, W=16, near=0.05, far=5.0, trunc=0.3, step=0.15, mw=1.0,
                 depth=p(outs["depth"][0]), vid=p(outs["vid"][0]), normal=p(outs["normal"][0]),
                 rgb_out=p(outs["rgb"][0]), label=p(outs["label"][0]), max_pixels=2 * 12 * 16,
                 ws=p(ws), ws_bytes=nb, flags=0, stream=None)

    def rr(**kw):
        return l.ucsa_tsdf_raycast(*{**rbase, **kw}.values())
    for kw, code in ((dict(tsdf=None), 0), (dict(weight=None), 1), (dict(rgb=None), 2),
                     (dict(rgb_out=None), 25), (dict(labels=None), 3), (dict(label=None), 26),
                     (dict(nx=1), 4), (dict(spacing=None), 8), (dict(poses=None), 9),
                     (dict(B=0), 10), (dict(near=0.0), 17), (dict(near=-1.0), 17),
                     (dict(far=0.01), 18), (dict(trunc=0.0), 19), (dict(step=0.3), 20),
                     (dict(step=0.5), 20), (dict(step=0.0), 20), (dict(mw=0.0), 21),
                     (dict(depth=None), 22), (dict(vid=None), 23),
                     (dict(max_pixels=2 * 12 * 16 - 1), 27), (dict(ws=None), 28),
                     (dict(ws_bytes=nb - 1), 29), (dict(flags=2), 30)):
        assert rr(**kw) == -1000 - code, (kw, code)
    torch.cuda.synchronize()
    for t, c in list(outs.values()) + [(ws, wcheck)]:
        c()
        assert (t == (9 if t.dtype == torch.uint8 else 5)).all()   # nothing was written
    assert rr() == 0 and rr(flags=1, ws=None, ws_bytes=0) == 0
    assert rr(normal=None) == 0 and rr(rgb=None, rgb_out=None, labels=None, label=None) == 0
    torch.cuda.synchronize()
    for t, c in list(outs.values()) + [(ws, wcheck)]:
        c()
    vcheck()
    z = outs["depth"][0].cpu().numpy()
    assert (z > 0).any() and np.abs(z[z > 0] - 0.45).max() < 0.06  # the step in tsdf at k = 4.5
    # ops
    v = ops.tsdf_volume(dims, (0, 0, 0), 0.1)
    with pytest.raises(UcsaError):
        ops.voxel_votes(v, 0)
    with pytest.raises(UcsaError):
        ops.voxel_votes(v, 256)
    vt = ops.voxel_votes(v, 5)
    assert vt.dtype == torch.uint16 and tuple(vt.shape) == (6,) + dims and not vt.cpu().numpy().any()
    intr = (10.0, 10.0, 8.0, 6.0)
    with pytest.raises(UcsaError):
        ops.vote_voxel_labels(vt, v, depth, pred.cpu(), poses, intr, 0.3)
    with pytest.raises(UcsaError):
        ops.vote_voxel_labels(vt, v, depth, pred.int(), poses, intr, 0.3)
    with pytest.raises(UcsaError):
        ops.vote_voxel_labels(vt[:, :4], v, depth, pred, poses, intr, 0.3)
    with pytest.raises(UcsaError):
        ops.vote_voxel_labels(vt, v, depth, pred, poses, intr, 0.0)
    with pytest.raises(UcsaError):
        ops.resolve_voxel_labels(vt, 0)
    with pytest.raises(UcsaError):
        ops.raycast_tsdf(v, poses, intr, 12, 16, 0.05, 5.0)          # no trunc anywhere
    with pytest.raises(UcsaError):
        ops.raycast_tsdf(v, poses, intr, 12, 16, 0.05, 5.0, step=0.3, trunc=0.3)
    with pytest.raises(UcsaError):
        ops.raycast_tsdf(v, poses, intr, 12, 16, 0.0, 5.0, trunc=0.3)
    with pytest.raises(UcsaError):
        ops.raycast_tsdf(v, poses, intr, 12, 16, 0.05, 5.0, trunc=0.3,
                         voxel_labels=torch.zeros(dims, dtype=torch.int32, device="cuda"))
    assert ops.vote_voxel_labels(vt, v, depth, pred, poses, intr, 0.3) is vt
    out = ops.raycast_tsdf(dict(v, trunc=0.3), poses, intr, 12, 16, 0.05, 5.0)
    assert sorted(out) == ["depth", "normal", "voxel_id"] and (out["voxel_id"] == -1).all()


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_script_end_to_end_from_a_scene_directory(tmp_path, capsys):
    from scripts import voxel_map_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    H, W, n = 240, 320, 16
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=H, W=W)
    dims, origin, h, trunc = room_volume_spec(128)
    out_dir = str(tmp_path / "maps")
    capsys.readouterr()
    rec = voxel_map_labels.main(
        ["--scene_root", sroot, "--labels", "label_40", "--out_dir", out_dir, "--voxel",
         repr(float(h)), "--step", repr(0.5 * float(h)), "--score", "--aabb", "-3.05", "-3.05",
         "-3.05", "3.05", "3.05", "3.05"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == n and line["dims"] == [128, 128, 128]
    assert line["voxel_map"] == rec["voxel_map"] and line["input"]["mIoU"] > 0.999
    with capsys.disabled():
        print(f"\nvoxel map from the scene directory: mIoU {rec['voxel_map']['mIoU']:.4f} "
              f"(accuracy {rec['voxel_map']['total_acc']:.4f}), input "
              f"{rec['input']['mIoU']:.4f}; fuse {rec['fuse_ms_per_view']} ms/view, ray-cast "
              f"{rec['raycast_ms_per_view']} ms/view")
    assert rec["voxel_map"]["mIoU"] >= MIOU_MIN and rec["voxel_map"]["total_acc"] >= ACC_MIN
    tol = float(trunc)
    for b in range(n):
        stem = f"{b:06d}"
        lab = _png(os.path.join(out_dir, "map_label", stem + ".png"))
        mm = _png(os.path.join(out_dir, "map_depth", stem + ".png"))
        assert lab.dtype == np.uint8 and lab.shape == (H, W) and mm.dtype == np.uint16
        z = mm.astype(np.float32) / np.float32(1000.0)
        png = _png(os.path.join(sroot, "depth", stem + ".png")).astype(np.float32) / \
            np.float32(1000.0)
        have = png > 0
        both = have & (z > 0)
        assert both.sum() / have.sum() >= COVER_MIN
        assert (np.abs(z[both] - png[both]) > tol).mean() <= DISAGREE_MAX
        assert ((lab > 0) <= (z > 0)).all()
    # every second frame, a higher vote threshold, the default box (padded by trunc) and step
    few = voxel_map_labels.main(["--scene_root", sroot, "--labels", "label_40", "--out_dir",
                                 str(tmp_path / "few"), "--voxel", repr(float(h)), "--every", "2",
                                 "--min_votes", "2", "--score"])
    assert few["frames"] == n // 2 and few["labelled"] < rec["labelled"]
    assert len(os.listdir(tmp_path / "few" / "map_label")) == n // 2
    assert few["voxel_map"]["pixels"] > 0
