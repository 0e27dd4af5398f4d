"""GPU: projective ICP (csrc/mesh_register.hip: ucsa_projective_icp_sums;
ops.register.projective_sums) and the depth pyramid (csrc/depth_frontend.hip:
ucsa_depth_pyramid_down; ops.depth.pyramid_down) against the restatement of
tests/projective_numpy.py, byte for byte: the 29 sums as int64 words, pixel,
the residuals as int32 words (NaNs included); the loops of
utils.registration (register_frames, refine_pose_projective) against the
restatement's loops; argument errors; the script's two flags.  The inputs and
the gates are those of tests/test_projective_cpu.py (figures:
docs/DESIGN_NOTEBOOK.md, PJ)."""
import json

import numpy as np
import pytest
import torch

from tests import depth_numpy as DN
from tests import projective_numpy as PJ
from tests.test_gpu_tsdf_fusion import _ops
from tests.test_gpu_tsdf_register import gpu_volume
from tests.test_projective_cpu import (ROOM_PAIRS, SR_FAR, SR_ITERATIONS, SR_MEASURED, SR_NEAR,
                                       edge_rows, look_at, render_room, sr_filter, sr_volume)
from tests.test_register_cpu import bits, pose_error, rigid
from tests.test_tsdf_register_cpu import SR_HELD, held_out_start, synthetic_case
from ucsa_neural_rendering_amd.utils import registration as REG
from ucsa_neural_rendering_amd.utils.registration import compose

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 0x5A


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()


def words(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- the step -------------------------------------------------------------------
MAPS = {"1x1": (1, 1, (1.3, 1.1, 0.4, 0.7)), "3x2": (3, 2, (2.5, 3.0, 0.8, 1.9)),
        "17x33": (17, 33, (21.0, 19.5, 14.3, 9.6))}        # principal points off the centre
SIZES = [0, 1, 255, 256, 257, 65537]                       # 65 537: three reduce stages
TRANSFORMS = {"identity": np.eye(4), "3deg": rigid(3.0, 0.05), "170deg": rigid(170.0, 0.3, seed=3)}


def target_maps(name):
    """a wavy surface through ``depth_normals``' restatement, with unmeasured pixels,
    every mask bit present, and a NaN and an inf planted in a point and a normal"""
    H, W, K = MAPS[name]
    g = np.random.default_rng(H * W)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    depth = (2.0 + 0.3 * np.sin(0.7 * i + 0.2) * np.cos(0.5 * j) + 0.02 * g.random((H, W))).astype(F)
    if H * W > 6:
        depth[2:4, 5:9] = 0.0
        depth[10:, 20:] += F(0.8)                          # a depth edge
    tp, tn, tm = (a[0].copy() for a in DN.normals_vec(depth[None], K, 0.25, 0.0, 0.995))
    if H * W == 1:                                         # a lone pixel has no normal of its own
        tn[0, 0], tm[0, 0] = (0.0, 0.0, -1.0), 3
    if H * W == 6:
        tn[...] = np.array([0.0, 0.6, -0.8], F)
        tm[...] = np.array([[3, 7], [11, 1], [15, 3]], np.uint8)
    if H * W > 6:
        tp[7, 7, 1], tn[8, 8, 0], tp[9, 9, 2], tn[6, 6, 2] = np.nan, np.nan, np.inf, -np.inf
    return tp, tn, tm, K


def source_points(tp, n, T, seed):
    """``n`` source rows whose moved positions lie on, near and far from the target's
    points, outside the image, behind the camera, and NaN / inf rows"""
    g = np.random.default_rng(seed)
    flat = tp.reshape(-1, 3)
    base = np.nan_to_num(flat[g.integers(0, flat.shape[0], n)], nan=1.0, posinf=2.0, neginf=2.0)
    world = (base + g.normal(0, 0.08, (n, 3)) * (g.random((n, 1)) < 0.8)).astype(F)
    kind = g.integers(0, 10, n)
    world[kind == 0] *= F(3.0)                                       # off the image
    world[kind == 1, 2] *= F(-1.0)                                   # behind the camera
    world[kind == 2, 2] = F(0.0)
    if n >= 255:
        world[5], world[17, 1], world[40, 2], world[41] = np.nan, np.inf, -np.inf, np.inf
    with np.errstate(all="ignore"):
        src = ((world.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(F)
    nrm = g.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    nrm[kind >= 5] = (np.array([0.0, 0.0, -1.0]) @ T[:3, :3]).astype(F)   # many compatible ones
    return src, nrm


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(MAPS))
def test_sums_pixels_and_residuals_equal_the_restatement_byte_for_byte(name, n):
    ops = _ops()
    tp, tn, tm, K = target_maps(name)
    gtp, gtn, gtm = _cu(tp), _cu(tn), _cu(tm)
    checked, matched_rows = 0, 0
    for tname, T in TRANSFORMS.items():
        src, nrm = source_points(tp, n, T, 300 + n)
        perm = np.random.default_rng(n).permutation(n)
        for order in ("given", "shuffled"):
            if order == "shuffled":
                src, nrm = src[perm], nrm[perm]
            gsrc, gnrm = _cu(src), _cu(nrm)
            for normals, gnormals in ((None, None), (nrm, gnrm)):
                for max_dist in (0.3, 0.05):
                    for min_cos in (0.0, 0.8):
                        for reject in (12, 4):
                            ref = PJ.projective_sums(src, normals, tp, tn, tm, K, T, max_dist,
                                                     min_cos, reject)
                            got = ops.register.projective_sums(
                                gsrc, gnormals, gtp, gtn, gtm, K, T, max_dist, min_cos, reject,
                                return_matches=True)
                            again = ops.register.projective_sums(gsrc, gnormals, gtp, gtn, gtm, K,
                                                                 T, max_dist, min_cos, reject)
                            what = (name, n, tname, order, normals is not None, max_dist, min_cos,
                                    reject)
                            s = got[0].cpu().numpy()
                            assert bits(s).tolist() == bits(ref[0]).tolist(), what
                            assert np.array_equal(got[1].cpu().numpy(), ref[1]), what
                            assert np.array_equal(words(got[2].cpu().numpy()), words(ref[2])), what
                            assert torch.equal(again.view(torch.int64), got[0].view(torch.int64))
                            checked += 1
                            matched_rows += int(ref[0][28])
            # the inputs are untouched
            assert np.array_equal(words(gsrc.cpu().numpy()), words(src))
            assert np.array_equal(words(gnrm.cpu().numpy()), words(nrm))
    for g_, h_ in ((gtp, tp), (gtn, tn)):
        assert np.array_equal(words(g_.cpu().numpy()), words(h_))
    assert np.array_equal(gtm.cpu().numpy(), tm)
    assert checked == 3 * 2 * 2 * 2 * 2 * 2
    if n >= 255:
        assert matched_rows > 0                   # the grid is not all unmatched rows


def test_the_edge_rows_of_the_cpu_test_fall_in_the_same_pixels():
    ops = _ops()
    pts, nrm, tp, tn, tm, K, md, mc, want = edge_rows()
    for normals in (nrm, None):
        ref = PJ.projective_sums(pts, normals, tp, tn, tm, K, np.eye(4), md, mc)
        got = ops.register.projective_sums(_cu(pts), None if normals is None else _cu(normals),
                                           _cu(tp), _cu(tn), _cu(tm), K, np.eye(4), md, mc,
                                           return_matches=True)
        assert got[1].cpu().tolist() == ref[1].tolist()
        assert np.array_equal(words(got[2].cpu().numpy()), words(ref[2]))
        assert bits(got[0].cpu().numpy()).tolist() == bits(ref[0]).tolist()
    assert ref[1][-3:].tolist() == [6, 6, 6] and got[1].cpu()[:-3].tolist() == want[:-3].tolist()
    bad = want < 0
    sums = ops.register.projective_sums(_cu(pts[bad]), _cu(nrm[bad]), _cu(tp), _cu(tn), _cu(tm), K,
                                        np.eye(4), md, mc)
    assert sums.cpu().view(torch.int64).tolist() == [0] * 29       # +0.0, not -0.0, not NaN


def test_guard_words_around_the_outputs_survive_and_arguments_come_before_any_launch():
    import ctypes as C

    from ucsa_neural_rendering_amd import _lib
    tp, tn, tm, K = target_maps("17x33")
    H, W = tm.shape
    n = 257
    src, nrm = source_points(tp, n, np.eye(4), 1)
    gsrc, gnrm, gtp, gtn, gtm = _cu(src), _cu(nrm), _cu(tp), _cu(tn), _cu(tm)
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    pad = 64
    buf = {k: torch.full((size + 2 * pad,), GUARD, dtype=torch.uint8, device="cuda")
           for k, size in (("sums", 29 * 8), ("pixel", 4 * n), ("residual", 4 * n),
                           ("ws", 8 * 29 * 2))}
    inner = lambda k: buf[k][pad:-pad]
    T12 = (C.c_float * 12)(*np.eye(4)[:3].reshape(-1))

    def raw(**over):
        a = dict(points=gsrc, normals=gnrm, n=n, tp=gtp, tn=gtn, tm=gtm, H=H, W=W, reject=12,
                 fx=K[0], fy=K[1], cx=K[2], cy=K[3], T=T12, md=0.3, mc=0.5, ws=inner("ws"),
                 wsn=29 * 2, sums=inner("sums"), pixel=inner("pixel"), residual=inner("residual"))
        a.update(over)
        return l.ucsa_projective_icp_sums(
            p(a["points"]), p(a["normals"]), a["n"], p(a["tp"]), p(a["tn"]), p(a["tm"]), a["H"],
            a["W"], a["reject"], a["fx"], a["fy"], a["cx"], a["cy"], a["T"], a["md"], a["mc"],
            p(a["ws"]), a["wsn"], p(a["sums"]), p(a["pixel"]), p(a["residual"]), None)
    nan, inf = float("nan"), float("inf")
    assert raw(points=None) == -1000 and raw(n=0x80000000) == -1002
    assert raw(tp=None) == -1003 and raw(tn=None) == -1004 and raw(tm=None) == -1005
    assert raw(H=0) == -1006 and raw(H=16385) == -1006 and raw(W=0) == -1007
    assert raw(W=16385) == -1007 and raw(reject=1) == -1008 and raw(reject=16) == -1008
    assert raw(fx=0.0) == -1009 and raw(fx=inf) == -1009 and raw(fy=-1.0) == -1010
    assert raw(fy=nan) == -1010 and raw(cx=nan) == -1011 and raw(cy=inf) == -1012
    assert raw(T=None) == -1013 and raw(md=0.0) == -1014 and raw(md=nan) == -1014
    assert raw(md=2e19) == -1014 and raw(mc=1.5) == -1015 and raw(mc=nan) == -1015
    assert raw(ws=None) == -1016 and raw(wsn=29 * 2 - 1) == -1017 and raw(sums=None) == -1018
    torch.cuda.synchronize()
    assert all(bool((b == GUARD).all()) for b in buf.values())     # nothing was written
    assert raw() == 0
    torch.cuda.synchronize()
    for b in buf.values():
        assert bool((b[:pad] == GUARD).all()) and bool((b[-pad:] == GUARD).all())
    ref = PJ.projective_sums(src, nrm, tp, tn, tm, K, np.eye(4), 0.3, 0.5, 12)
    assert inner("sums").cpu().view(torch.int64).tolist() == bits(ref[0]).tolist()
    assert inner("pixel").cpu().view(torch.int32).tolist() == ref[1].tolist()
    assert np.array_equal(inner("residual").cpu().view(torch.int32).numpy(), words(ref[2]))
    # the optional outputs may be NULL, and so may the normals
    assert raw(pixel=None, residual=None, normals=None) == 0
    torch.cuda.synchronize()


def test_the_op_checks_its_arguments_before_the_library(monkeypatch):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    tp, tn, tm, K = target_maps("3x2")
    src, nrm = source_points(tp, 10, np.eye(4), 0)
    gsrc, gnrm, gtp, gtn, gtm = _cu(src), _cu(nrm), _cu(tp), _cu(tn), _cu(tm)
    T = np.eye(4)

    def boom(*a, **k):
        raise AssertionError("the op reached lib()")
    monkeypatch.setattr(ops.register, "lib", boom)
    monkeypatch.setattr(ops.depth, "lib", boom)
    call = ops.register.projective_sums
    bad = [lambda: call(gsrc.cpu(), gnrm, gtp, gtn, gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm[:5], gtp, gtn, gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm.double(), gtp, gtn, gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm, gtp.cpu(), gtn, gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn[:1], gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm.int(), K, T, 0.3),
           lambda: call(gsrc, gnrm, gtp.reshape(-1, 3), gtn, gtm, K, T, 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, (0.0, 1.0, 0.0, 0.0), T, 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, (1.0, 1.0, float("nan"), 0.0), T, 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, K, np.eye(3), 0.3),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, K, T, 0.0),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, K, T, 0.3, min_cos=1.5),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, K, T, 0.3, reject=1),
           lambda: call(gsrc, gnrm, gtp, gtn, gtm, K, T, 0.3, reject=True),
           lambda: ops.depth.pyramid_down(gtp[..., 0].cpu()[None], 0.1),
           lambda: ops.depth.pyramid_down(gtp[..., 0], 0.1),
           lambda: ops.depth.pyramid_down(gtp[..., 0][None], -0.1),
           lambda: ops.depth.pyramid_down(gtp[..., 0][None], 0.1, float("inf")),
           lambda: ops.depth.pyramid_down(gtp[..., 0][None], 0.1, depth_min=2.0, depth_max=1.0)]
    for c in bad:
        with pytest.raises(_lib.UcsaError):
            c()


# ---- the pyramid ---------------------------------------------------------------------
def pyramid_frames(B, H, W):
    """measured depths with steps, and every kind of pixel that is no measurement;
    depth_min = 0.5 and depth_max = 4 exactly present; in the frames large enough a
    member exactly thr = 0.25 from z0 and one a step beyond"""
    g = np.random.default_rng(B * 1000 + H * W)
    d = (1.0 + 2.0 * g.random((B, H, W))).astype(F)
    d[g.random((B, H, W)) < 0.15] = 0.0
    flat = d.reshape(-1)
    specials = [np.nan, np.inf, -np.inf, -1.5, 0.5, 4.0, np.nextafter(F(0.5), F(0)),
                np.nextafter(F(4.0), F(5))]
    for k, v in enumerate(specials[:flat.size]):
        flat[(k * 7) % flat.size] = v
    if H >= 4 and W >= 4:
        d[:, 2, 2:4] = (1.0, 1.25)
        d[:, 3, 2:4] = (np.nextafter(F(1.25), F(2)), 1.125)
    return d


@pytest.mark.parametrize("B", [1, 3])
def test_pyramid_down_equals_the_restatement_word_for_word(B):
    ops = _ops()
    for H, W in ((1, 1), (2, 2), (3, 2), (17, 33)):
        d = pyramid_frames(B, H, W)
        gd = _cu(d)
        for max_jump, z2 in ((0.25, 0.0), (0.0, 0.0), (0.05, 0.02)):
            ref = PJ.pyramid_down(d, max_jump, z2, 0.5, 4.0)
            got = ops.depth.pyramid_down(gd, max_jump, z2, 0.5, 4.0)
            assert got.shape == ref.shape and got.dtype == torch.float32
            assert np.array_equal(words(got.cpu().numpy()), words(ref)), (B, H, W, max_jump, z2)
            assert torch.equal(ops.depth.pyramid_down(gd, max_jump, z2, 0.5, 4.0).view(torch.int32),
                               got.view(torch.int32))
        assert np.array_equal(words(gd.cpu().numpy()), words(d))     # the input is untouched
    # the library's own codes, before any launch
    import ctypes as C

    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    out = torch.full((B * 9 * 17 + 32,), 7.0, device="cuda")
    raw = lambda depth=gd, b=B, h=17, w=33, mj=0.1, z2=0.0, lo=0.5, hi=4.0, o=out: \
        l.ucsa_depth_pyramid_down(p(depth), b, h, w, mj, z2, lo, hi, p(o), None)
    nan = float("nan")
    assert raw(depth=None) == -1000 and raw(b=0) == -1001 and raw(h=0) == -1002
    assert raw(w=16385) == -1003 and raw(mj=-1.0) == -1004 and raw(z2=nan) == -1005
    assert raw(lo=nan) == -1006 and raw(hi=0.25) == -1007 and raw(o=None) == -1008
    assert raw(o=gd) == -1008
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert bool((out[B * 9 * 17:] == 7.0).all())                      # nothing past the frames


# ---- the loops -----------------------------------------------------------------------
LOOP_H, LOOP_W, LOOP_K = 24, 32, (24.0, 24.0, 16.0, 12.0)


def small_room(pose):
    return render_room(pose, LOOP_H, LOOP_W, LOOP_K)


def test_register_frames_equals_the_restatements_loop_bit_for_bit():
    from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter
    eye, target, motion = ROOM_PAIRS["pillar"]
    dst_pose = look_at(eye, target).astype(np.float64)
    src_pose = dst_pose @ compose(np.eye(4), np.asarray(motion))
    z_src, z_dst = small_room(src_pose), small_room(dst_pose)
    flt = DepthFilter(max_jump=0.15)                       # a 24 x 32 pixel is 0.04 to 0.12 wide
    for filtered in (False, True):
        ref_src = PJ.frame_maps(z_src, LOOP_K, flt, 3, filtered)
        ref_dst = PJ.frame_maps(z_dst, LOOP_K, flt, 3, filtered)
        src = REG.frame_maps(z_src, LOOP_K, flt, 3, filtered)
        dst = REG.frame_maps(z_dst, LOOP_K, flt, 3, filtered)
        for level in range(3):
            for key in ("depth", "points", "normals"):
                assert np.array_equal(words(src[level][key].cpu().numpy()),
                                      words(ref_src[level][key])), (filtered, level, key)
            assert np.array_equal(dst[level]["mask"].cpu().numpy(), ref_dst[level]["mask"])
            assert src[level]["intrinsics"] == ref_src[level]["intrinsics"]
        start = compose(np.eye(4), np.array([0.02, -0.01, 0.015, 0.03, 0.02, -0.02]))
        for its in ((4, 3, 2), (5,)):
            ref = PJ.register_frames(ref_src, ref_dst, LOOP_K, init=start, iterations=its)
            got = REG.register_frames(src, dst, LOOP_K, init=start, iterations=its)
            assert ref["matched"] > 100 and ref["rank"] == 6
            assert [h["level"] for h in got["history"]] == [h["level"] for h in ref["history"]]
            for a, b in zip(got["history"], ref["history"]):
                assert bits(a["sums"]).tolist() == bits(b["sums"]).tolist()
            assert bits(got["transform"]).tolist() == bits(ref["transform"]).tolist()
            for key in ("matched", "rank", "iterations", "converged", "n_points"):
                assert got[key] == ref[key], key


def test_odometry_chains_the_pairs_and_counts_a_frame_without_a_measurement():
    from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter
    eye, target, motion = ROOM_PAIRS["pillar"]
    first = look_at(eye, target).astype(np.float64)
    step = compose(np.eye(4), np.asarray(motion))
    frames = [small_room(first), small_room(first @ step), np.zeros((LOOP_H, LOOP_W), F)]
    flt = DepthFilter(max_jump=0.15)
    ref = PJ.odometry(frames, LOOP_K, flt, filtered=False, iterations=(4, 3))
    got = REG.odometry(frames, LOOP_K, flt, filtered=False, iterations=(4, 3))
    assert bits(got["poses"]).tolist() == bits(ref[0]).tolist()
    assert got["fallbacks"] == ref[2] == 1 and got["records"][0] is None
    assert [r["fallback"] for r in got["records"][1:]] == [False, True]
    assert got["records"][1]["rank"] == 6


def test_refine_pose_projective_against_the_fused_room_ends_within_the_recorded_gate():
    case = synthetic_case()
    vol = gpu_volume(sr_volume())
    seed = 0
    true, start = held_out_start(case, seed)
    out = REG.refine_pose_projective(case["depth"][SR_HELD], start, case["intr"], vol,
                                     case["trunc"], iterations=SR_ITERATIONS, near=SR_NEAR,
                                     far=SR_FAR, depth_filter=sr_filter(), filtered=False)
    rot, trans = pose_error(out["pose"], true)
    print(f"rot {rot:.4e} rad, trans {trans:.4e}, matched {out['matched']} of {out['n_points']}")
    assert out["rank"] == 6 and out["n_points"] == 768
    assert rot <= 2 * SR_MEASURED[seed][0] and trans <= 2 * SR_MEASURED[seed][1]
    assert bits(out["pose"]).tolist() == bits(start @ out["transform"]).tolist()


# ---- the script --------------------------------------------------------------------------
def test_the_script_tracks_projectively_walks_without_poses_and_is_unchanged_without_the_flags(
        tmp_path, capsys):
    from scripts import fuse_tsdf_mesh
    from tests.test_gpu_tsdf_register import BOX
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=6, H=48, W=64)
    box = ["--voxel", "0.1", "--aabb"] + [str(v) for v in BOX] + ["--no_color"]
    capsys.readouterr()
    plain = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "a.ply")] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == plain
    assert sorted(plain) == ["dims", "extract_ms", "faces", "frames", "integrate_ms_per_view",
                             "observed", "origin", "out", "vertices", "voxel"]
    # --refine_method tsdf is the default: the same bytes as --refine_poses alone
    t1 = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "b.ply"),
                              "--refine_poses", "--refine_iters", "5"] + box)
    t2 = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "c.ply"),
                              "--refine_poses", "--refine_iters", "5", "--refine_method", "tsdf"]
                             + box)
    capsys.readouterr()
    assert t1["refine"] == t2["refine"]
    assert open(tmp_path / "b.ply", "rb").read() == open(tmp_path / "c.ply", "rb").read()
    out = str(tmp_path / "poses" / "used.npy")
    rec = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "d.ply"),
                               "--refine_poses", "--refine_iters", "5", "--refine_method",
                               "projective", "--depth_filter", "max_jump=0.15",
                               "--poses_out", out] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert [l.split(":")[0] for l in lines[:-1]] == ["depth_filter", "refine"]
    assert rec["refine"]["refined"] == 5 and 0 <= rec["refine"]["fallbacks"] <= 5
    assert np.load(out).shape == (6, 4, 4)
    assert read_ply(str(tmp_path / "d.ply"))["verts"].shape[0] > 1000
    rec = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "e.ply"),
                               "--odometry", "--depth_filter", "max_jump=0.15", "--poses_out", out]
                              + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert [l.split(":")[0] for l in lines[:-1]] == ["odometry", "depth_filter"]
    walked = json.loads(lines[0][len("odometry: "):])
    assert walked == rec["odometry"] and walked["frames"] == 6
    assert sorted(walked) == ["fallbacks", "frames", "matched_median", "rmse_median"]
    poses = np.load(out)
    assert poses.shape == (6, 4, 4) and poses.dtype == np.float64
    with pytest.raises(SystemExit):
        fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", str(tmp_path / "f.ply"),
                             "--refine_poses", "--refine_method", "projective",
                             "--refine_stride", "2"] + box)
