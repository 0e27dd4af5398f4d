"""GPU: view weights (ucsa_depth_confidence in csrc/depth_frontend.hip,
ucsa_tsdf_integrate_weighted in csrc/tsdf_fusion.hip) against the numpy
restatement of their contracts (tests/weighted_numpy.py), as int32 / uint8
words; weights of one against ops.integrate_tsdf; every batch size; untouched
voxels, guard words, argument codes; and the weights inside the fusion and the
script, end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_numpy as DN
from tests import tsdf_numpy as TN
from tests import weighted_numpy as WN
from tests.test_gpu_depth_frontend import K_OFF, frames, words
from tests.test_gpu_tsdf_fusion import guarded_volume
from tests.test_tsdf_fusion_cpu import (batches, random_case, room_volume_spec, run_numpy,
                                        same_bytes)
from tests.test_weighted_fusion_cpu import (COS_FLOOR, FILTER, least_weight, noisy_room_frontend,
                                            random_weights, run_weighted_numpy)

pytestmark = pytest.mark.gpu

F32 = np.float32


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# the confidence map
# ---------------------------------------------------------------------------
def gpu_normals(z, K, max_jump, **kw):
    """ops.depth.depth_normals of ``z`` -> (points, normals, mask) tensors; held to
    the restatement, so that the confidence test's inputs are what they claim"""
    out = _ops().depth.depth_normals(_cu(z), K, max_jump, **kw)
    want = DN.normals(z, K, max_jump, **kw)
    for got, w in zip((out["points"], out["normals"], out["mask"]), want):
        assert np.array_equal(words(got), words(w))
    return out["points"], out["normals"], out["mask"]


def check_confidence(pts, nrm, mask, *args, **kw):
    ops = _ops()
    before = [t.clone() for t in (pts, nrm, mask)]
    got = ops.depth.depth_confidence(pts, nrm, mask, *args, **kw)
    again = ops.depth.depth_confidence(pts, nrm, mask, *args, **kw)
    torch.cuda.synchronize()
    want = WN.confidence(pts.cpu().numpy(), nrm.cpu().numpy(), mask.cpu().numpy(), *args, **kw)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(words(got), words(want))
    assert np.array_equal(words(got), words(again))
    for t, b in zip((pts, nrm, mask), before):
        assert torch.equal(t, b), "an input was written"
    return want


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 1, 1), (1, 3, 2), (3, 3, 2), (1, 17, 33),
                                   (3, 17, 33)])
def test_confidence_is_the_restatements_words(shape):
    """frames with NaN, +-inf, 0 and negative pixels, two levels (edges) and a
    ramp, a strict min_cos (grazing): every mask value; reject sets; sigma_z2 = 0
    and > 0"""
    dmin, dmax = 1.25, 3.0
    z = frames(sum(shape), *shape, dmin, dmax)
    pts, nrm, mask = gpu_normals(z, K_OFF, 0.09, max_jump_z2=0.003, min_cos=0.93, depth_min=dmin,
                                 depth_max=dmax)
    m = mask.cpu().numpy()
    if shape[1] >= 13:
        assert set(np.unique(m)) >= {0, 1, 3, 5, 7, 11, 15}
    for reject in (12, 4, 8, 0):
        for s2 in (0.0, 0.02):
            w = check_confidence(pts, nrm, mask, 0.05, s2, 0.3, reject)
            keep = ((m & 1) != 0) & ((m & reject) == 0)
            assert ((w > 0) == keep).all() and w.max(initial=0.0) <= 1.0
            if s2 == 0.0:
                assert (w[keep & ((m & 2) == 0)] == F32(0.3)).all()
                assert (w[keep] >= F32(0.3)).all()


def restated_cosv(pts, nrm):
    p, n = pts.astype(F32), nrm.astype(F32)
    dot = (n[..., 0] * p[..., 0] + n[..., 1] * p[..., 1]) + n[..., 2] * p[..., 2]
    return (-dot) / np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1])
                            + p[..., 2] * p[..., 2])


def test_cos_floor_exactly_at_a_pixels_cosine_and_one_ulp_to_either_side():
    z = (2.0 + 0.01 * np.arange(33, dtype=F32))[None, None, :].repeat(17, 1)
    pts, nrm, mask = gpu_normals(z, K_OFF, 0.5)
    assert (mask == 3).all()
    cosv = restated_cosv(pts.cpu().numpy(), nrm.cpu().numpy())
    c = cosv[0, 8, 20]
    assert 0.5 < c < 0.9999
    for floor, expect in ((c, c), (np.nextafter(c, F32(2)), np.nextafter(c, F32(2))),
                          (np.nextafter(c, F32(0)), c)):
        w = check_confidence(pts, nrm, mask, 0.05, 0.0, float(floor))   # sigma_z2 = 0: w = wa
        assert w[0, 8, 20] == expect
        assert (w >= floor).all() and (w == floor).any() and (w > floor).any()


def test_a_cosine_above_one_by_rounding_is_clamped_and_a_nan_takes_the_floor():
    """a sphere about the camera: every normal lies along its pixel's ray, cosv is
    1 up to rounding and above it at some pixels"""
    H, W = 17, 33
    j = (np.arange(W) + 0.5 - K_OFF[2]) / K_OFF[0]
    i = (np.arange(H) + 0.5 - K_OFF[3]) / K_OFF[1]
    z = (3.0 / np.sqrt(1 + j[None, :] ** 2 + i[:, None] ** 2))[None].astype(F32)
    pts, nrm, mask = gpu_normals(z, K_OFF, 0.5)
    cosv = restated_cosv(pts.cpu().numpy(), nrm.cpu().numpy())
    assert (cosv > 1).sum() >= 3 and (mask == 3).all()
    w = check_confidence(pts, nrm, mask, 0.05, 0.0, 0.2)
    assert (w[cosv > 1] == 1.0).all() and w.max() == 1.0 and (w < 1).any()
    # hand-made inputs: a zero point under a NORMAL bit has cosv = 0/0
    p = torch.zeros(1, 1, 2, 3, device="cuda")
    p[0, 0, 1, 2] = 2.0
    n = torch.zeros_like(p)
    n[..., 2] = -1.0
    m = torch.full((1, 1, 2), 3, dtype=torch.uint8, device="cuda")
    w = check_confidence(p, n, m, 0.05, 0.0, 0.2)
    assert w[0, 0, 0] == F32(0.2) and w[0, 0, 1] == 1.0


def test_confidence_writes_nothing_else_and_checks_every_argument():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    B, H, W, G = 3, 17, 33, 1024
    z = frames(4, B, H, W, 1e-6, 3.0e38)
    pts, nrm, mask = gpu_normals(z, K_OFF, 0.09, min_cos=0.9)
    want = WN.confidence(pts.cpu().numpy(), nrm.cpu().numpy(), mask.cpu().numpy(), 0.05, 0.01,
                         0.1, 12)
    n = B * H * W
    buf = torch.full((2 * G + n,), -777.25, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    out = C.c_void_p(buf.data_ptr() + 4 * G)
    good = [p(pts), p(nrm), p(mask), B, H, W, 0.05, 0.01, 0.1, 12, out, None]
    nan, inf = float("nan"), float("inf")
    inside = lambda t, off: C.c_void_p(t.data_ptr() + off)
    for k, v in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (4, 16385), (5, 0), (5, 16385),
                 (6, 0.0), (6, -1.0), (6, nan), (6, inf), (7, -0.1), (7, nan), (7, inf),
                 (8, 0.0), (8, -0.5), (8, 1.5), (8, nan), (9, 1), (9, 2), (9, 16), (10, None),
                 (10, p(pts)), (10, p(nrm)), (10, p(mask)), (10, inside(pts, 8 * n)),
                 (10, inside(nrm, 12 * n - 4)), (10, inside(mask, n - 1))):
        args = list(good)
        args[k] = v
        assert l.ucsa_depth_confidence(*args) == -1000 - k, (k, v)
    torch.cuda.synchronize()
    assert (buf == -777.25).all()                      # nothing was launched
    assert l.ucsa_depth_confidence(*good) == 0
    torch.cuda.synchronize()
    assert (buf[:G] == -777.25).all() and (buf[-G:] == -777.25).all()
    assert np.array_equal(words(buf[G:-G]).reshape(-1), words(want).reshape(-1))
    # the wrapper refuses the same before the library is reached
    ops = _ops()
    for bad in (dict(sigma_depth=0.0), dict(sigma_z2=-1.0), dict(cos_floor=0.0),
                dict(cos_floor=1.5), dict(reject=3), dict(reject=True)):
        kw = dict(sigma_depth=0.05, sigma_z2=0.0, cos_floor=0.1, reject=12)
        kw.update(bad)
        with pytest.raises(_lib.UcsaError):
            ops.depth.depth_confidence(pts, nrm, mask, **kw)
    for bad in ((pts.cpu(), nrm, mask), (pts, nrm.cpu(), mask), (pts, nrm, mask.cpu()),
                (pts, nrm[:1], mask), (pts, nrm, mask.float()), (pts[..., :2], nrm, mask),
                (pts.cpu().numpy(), nrm, mask)):
        with pytest.raises(_lib.UcsaError):
            ops.depth.depth_confidence(*bad, 0.05)


# ---------------------------------------------------------------------------
# the weighted integration
# ---------------------------------------------------------------------------
def run_gpu(case, weights, splits, with_color=True, start=None):
    """the case integrated with ``weights`` (None: ops.integrate_tsdf) in calls of
    the views [a, b) of ``splits``, into guarded volumes that hold ``start``"""
    ops = _ops()
    vol, check = guarded_volume(case["dims"], case["origin"], case["spacing"], with_color)
    if start is not None:
        for k in ("tsdf", "weight", "rgb"):
            if vol[k] is not None:
                vol[k].copy_(_cu(start[k]))
    depth, poses, color = _cu(case["depth"]), _cu(case["poses"]), _cu(case["color"])
    pw = None if weights is None else _cu(weights)
    kw = dict(max_weight=case["max_weight"], depth_min=case["depth_min"],
              depth_max=case["depth_max"])
    for a, b in splits:
        col = color[a:b] if with_color else None
        if pw is None:
            ops.integrate_tsdf(vol, depth[a:b], poses[a:b], case["intr"], case["trunc"],
                               color=col, **kw)
        else:
            ops.depth.integrate_tsdf_weighted(vol, depth[a:b], pw[a:b], poses[a:b], case["intr"],
                                              case["trunc"], color=col, **kw)
    torch.cuda.synchronize()
    check()
    return {k: (None if vol[k] is None else vol[k].cpu().numpy())
            for k in ("tsdf", "weight", "rgb")}


@pytest.fixture(scope="module")
def case16():
    case = random_case(0, views=16)
    w = random_weights(case)
    return case, w, run_weighted_numpy(case, w, [(0, 16)])


def test_random_case_bit_exact_for_every_batch_size_and_twice(case16):
    """37 x 20 x 65 voxels, 48 x 64 frames, cameras inside, outside and looking
    away, invalid depth; weights 0, -1, NaN, +inf, a denormal, 1, in (0, 1) and
    above 1; max_weight = 11 saturates"""
    case, w, want = case16
    assert want["weight"].max() == 11.0 and 0.2 < (want["weight"] > 0).mean() < 1.0
    for size in list(range(1, 17)) + [16]:
        got = run_gpu(case, w, batches(16, size))
        for k in ("tsdf", "weight", "rgb"):
            assert got[k].tobytes() == want[k].tobytes(), (size, k)
    for splits in ([(0, 1), (1, 16)], [(0, 15), (15, 16)], [(0, 3), (3, 4), (4, 11), (11, 16)]):
        assert same_bytes(run_gpu(case, w, splits), want), splits
    plain = run_gpu(case, w, [(0, 16)], with_color=False)
    assert plain["rgb"] is None and plain["tsdf"].tobytes() == want["tsdf"].tobytes()
    assert plain["weight"].tobytes() == want["weight"].tobytes()


@pytest.mark.parametrize("views,color", [(1, True), (1, False), (33, True), (33, False)])
def test_one_view_and_more_views_than_one_launch_takes(views, color):
    case = random_case(3, views=views)       # 32 views per launch: 33 is two launches
    w = random_weights(case, 3)
    want = run_weighted_numpy(case, w, [(0, views)], with_color=color)
    assert (want["weight"] > 0).any()
    assert same_bytes(run_gpu(case, w, [(0, views)], with_color=color), want)


def test_weights_of_one_give_integrate_tsdfs_bytes(case16):
    case = case16[0]
    ones = np.ones(case["depth"].shape, F32)
    for color in (True, False):
        unweighted = run_gpu(case, None, [(0, 16)], with_color=color)
        assert same_bytes(unweighted, run_numpy(case, [(0, 16)], with_color=color))
        assert same_bytes(run_gpu(case, ones, [(0, 16)], with_color=color), unweighted)
        assert same_bytes(run_gpu(case, ones, batches(16, 5), with_color=color), unweighted)


def test_untouched_voxels_and_views_without_a_usable_weight_keep_the_bytes(case16):
    """the volumes start from a state with its own bit patterns (-0.0, a denormal
    weight); four views touch a part of it; then views whose weights are all 0,
    negative, NaN or inf"""
    case, w, _ = case16
    g = np.random.default_rng(21)
    start = TN.new_volume(case["dims"], case["origin"], case["spacing"], True)
    start["tsdf"][:] = g.uniform(-1, 1, start["tsdf"].shape).astype(F32)
    start["tsdf"][::3] = F32(-0.0)
    start["weight"][:] = g.uniform(0, 5, start["weight"].shape).astype(F32)
    start["weight"][1::4] = F32(1e-42)
    start["rgb"][:] = g.uniform(0, 255, start["rgb"].shape).astype(F32)
    want = {k: start[k].copy() for k in ("tsdf", "weight", "rgb")}
    want.update(origin=start["origin"], spacing=start["spacing"])
    sub = {**case, "depth": case["depth"][:4], "poses": case["poses"][:4],
           "color": case["color"][:4]}
    WN.integrate(want, sub["depth"], w[:4], sub["poses"], case["intr"], case["trunc"],
                 color=sub["color"], max_weight=case["max_weight"], depth_min=case["depth_min"],
                 depth_max=case["depth_max"])
    same = want["tsdf"].view(np.int32) == start["tsdf"].view(np.int32)
    assert 0.1 < same.mean() < 0.95
    got = run_gpu(sub, w[:4], [(0, 4)], start=start)
    assert same_bytes(got, want)
    for dead in (0.0, -1.0, np.nan, np.inf):
        assert same_bytes(run_gpu(sub, np.full_like(w[:4], dead), [(0, 2), (2, 4)], start=start),
                          start), dead


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    vol, check = guarded_volume((8, 9, 10), (0, 0, 0), 0.1, True)
    depth = torch.ones(2, 12, 16, device="cuda")
    pw = torch.full((2, 12, 16), 0.5, device="cuda")
    color = torch.zeros(2, 12, 16, 3, dtype=torch.uint8, device="cuda")
    poses = torch.eye(4, device="cuda").repeat(2, 1, 1).contiguous()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    o, h = _lib.fvec((0, 0, 0)), _lib.fvec((0.1, 0.1, 0.1))
    base = dict(tsdf=p(vol["tsdf"]), weight=p(vol["weight"]), rgb=p(vol["rgb"]), nx=8, ny=9,
                nz=10, origin=o, spacing=h, depth=p(depth), pixel_weight=p(pw), color=p(color),
                poses=p(poses), B=2, fx=10.0, fy=10.0, cx=8.0, cy=6.0, H=12, W=16, trunc=0.3,
                max_weight=10.0, depth_min=0.01, depth_max=5.0, stream=None)

    def rc(**kw):
        return l.ucsa_tsdf_integrate_weighted(*{**base, **kw}.values())

    before = {k: vol[k].clone() for k in ("tsdf", "weight", "rgb")}
    nan = float("nan")
    for kw, code in ((dict(tsdf=None), 0), (dict(weight=None), 1), (dict(rgb=None), 2),
                     (dict(color=None), 10), (dict(nx=1), 3), (dict(ny=1), 4), (dict(nz=1), 5),
                     (dict(nx=2048, ny=2048, nz=2048), 3), (dict(origin=None), 6),
                     (dict(spacing=None), 7), (dict(depth=None), 8),
                     (dict(pixel_weight=None), 9), (dict(poses=None), 11), (dict(B=0), 12),
                     (dict(fx=0.0), 13), (dict(fy=-1.0), 14), (dict(cx=nan), 15),
                     (dict(cy=nan), 16), (dict(H=0), 17), (dict(H=16385), 17),
                     (dict(W=0), 18), (dict(W=16385), 18), (dict(trunc=0.0), 19),
                     (dict(trunc=nan), 19), (dict(max_weight=0.5), 20),
                     (dict(depth_min=nan), 21), (dict(depth_max=0.001), 22)):
        assert rc(**kw) == -1000 - code, (kw, code)
    torch.cuda.synchronize()
    check()
    for k in before:
        assert torch.equal(vol[k], before[k])  # an argument error launches nothing
    assert rc() == 0 and rc(rgb=None, color=None) == 0
    torch.cuda.synchronize()
    check()
    assert (vol["weight"] > 0).any() and float(vol["weight"].max()) == 2.0   # 4 views at 0.5
    intr = (10.0, 10.0, 8.0, 6.0)
    v = ops.tsdf_volume((8, 9, 10), (0, 0, 0), 0.1, with_color=False)
    W_ = ops.depth.integrate_tsdf_weighted
    for bad in (lambda: W_(v, depth.cpu(), pw, poses, intr, 0.3),
                lambda: W_(v, depth, pw.cpu(), poses, intr, 0.3),
                lambda: W_(v, depth, pw.cpu().numpy(), poses, intr, 0.3),
                lambda: W_(v, depth, pw[:1], poses, intr, 0.3),
                lambda: W_(v, depth, pw.double(), poses, intr, 0.3),
                lambda: W_(v, depth, pw, poses.cpu(), intr, 0.3),
                lambda: W_({**v, "tsdf": v["tsdf"].cpu()}, depth, pw, poses, intr, 0.3),
                lambda: W_(v, depth, pw, poses, intr, 0.3, color=color),
                lambda: W_(v, depth, pw, poses[:1], intr, 0.3),
                lambda: W_(v, depth, pw, poses, intr, 0.0),
                lambda: W_(v, depth, pw, poses, intr, 0.3, max_weight=0.0)):
        with pytest.raises(UcsaError):
            bad()
    assert (v["weight"] == 0).all()
    assert W_(v, depth, pw, poses, intr, 0.3) is v


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
BOX = [-3.05] * 3 + [3.05] * 3


def test_fuse_depth_views_with_view_weights_gives_the_restatements_volume():
    """the CPU test's frames (tests/test_weighted_fusion_cpu.py, seed 0): the front
    end, the confidence map and the weighted integration on the GPU against the
    three restatements chained, as volume bytes and as the mesh's"""
    from ucsa_neural_rendering_amd.utils import depth_frontend as U
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import fuse_depth_views
    ops = _ops()
    room, poses, intr, noisy, fe = noisy_room_frontend(0)
    dims, origin, h, trunc = room_volume_spec(64)
    w = WN.confidence_vec(fe["points"], fe["normals"], fe["mask"], FILTER["sigma_depth"],
                          FILTER["sigma_z2"], COS_FLOOR)
    want = TN.new_volume(dims, origin, h)
    WN.integrate(want, fe["clean"], w, poses, intr, trunc)
    flt, vw = U.DepthFilter(**FILTER), U.ViewWeights()
    assert vw.cos_floor == COS_FLOOR and vw.resolved(flt) == (0.06, 0.006)
    # the pieces
    st, ws = U.new_stats(), U.new_weight_stats()
    clean, pw = U.weighted_depth(_cu(noisy), intr, flt, vw, stats=st, weight_stats=ws)
    assert np.array_equal(words(clean), words(fe["clean"])) and np.array_equal(words(pw), words(w))
    assert ws["kept"] == int((w > 0).sum()) == st["measured"] - st["rejected"]
    assert abs(ws["weight_sum"] - float(w.sum(dtype=np.float64))) < 1e-6 * ws["kept"]
    assert U.weight_stats_line(ws).startswith("view_weights: mean weight 0.08")
    vol = ops.tsdf_volume(dims, origin, float(h))
    for a, b in batches(16, 5):
        ops.depth.integrate_tsdf_weighted(vol, clean[a:b], pw[a:b], _cu(poses[a:b]), intr,
                                          float(trunc))
    assert np.array_equal(words(vol["tsdf"]), words(want["tsdf"]))
    assert np.array_equal(words(vol["weight"]), words(want["weight"]))
    # the whole: the mesh of that volume over the voxels seen at least once
    mw = 0.5 * least_weight(float(fe["clean"].max()))
    assert mw <= vw.least(flt, float(fe["clean"].max()))
    kw = dict(aabb=BOX, voxel=float(h), trunc=float(trunc))
    mesh = fuse_depth_views(poses, intr, 48, 64, noisy, depth_filter=flt, view_weights=vw,
                            min_weight=mw, batch=7, **kw)
    v, f, n = TN.extract(want, mw)
    assert mesh["dims"] == tuple(dims) and v.shape[0] > 5000
    assert mesh["verts"].tobytes() == v.tobytes() and mesh["faces"].tobytes() == f.tobytes()
    assert mesh["normals"].tobytes() == n.tobytes()
    assert mesh["view_weights"] == ws and mesh["depth_filter"] == st
    assert abs(mesh["observed"] - float((want["weight"] >= F32(mw)).mean())) < 1e-6
    # off is off: without the keyword the mesh is the unweighted one, and the
    # keyword without a filter is an error
    off = fuse_depth_views(poses, intr, 48, 64, noisy, depth_filter=flt, **kw)
    none = fuse_depth_views(poses, intr, 48, 64, noisy, depth_filter=flt, view_weights=None, **kw)
    plain = TN.new_volume(dims, origin, h)
    TN.integrate(plain, fe["clean"], poses, intr, trunc)
    pv, pf, pn = TN.extract(plain, 1.0)
    for m in (off, none):
        assert "view_weights" not in m
        assert m["verts"].tobytes() == pv.tobytes() and m["faces"].tobytes() == pf.tobytes()
    with pytest.raises(ValueError):
        fuse_depth_views(poses, intr, 48, 64, noisy, view_weights=vw, **kw)


def test_the_other_consumers_take_view_weights():
    """tracking, the occupancy prior and the voxel map integrate the same weighted
    volume; the vote table is the unweighted run's"""
    from ucsa_neural_rendering_amd.utils import depth_frontend as U
    from ucsa_neural_rendering_amd.utils.occupancy_prior import (prior_from_depth_views,
                                                                 volume_from_depth_views)
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import track_depth_views
    from ucsa_neural_rendering_amd.utils.voxel_map import fuse_semantic_views
    ops = _ops()
    room, poses, intr, noisy, fe = noisy_room_frontend(0)
    dims, origin, h, trunc = room_volume_spec(64)
    w = WN.confidence_vec(fe["points"], fe["normals"], fe["mask"], FILTER["sigma_depth"],
                          FILTER["sigma_z2"], COS_FLOOR)
    want = TN.new_volume(dims, origin, h)
    WN.integrate(want, fe["clean"], w, poses, intr, trunc)
    flt, vw = U.DepthFilter(**FILTER), U.ViewWeights()
    kw = dict(aabb=BOX, voxel=float(h), trunc=float(trunc))
    vol, _, _ = volume_from_depth_views(poses, intr, 48, 64, noisy, depth_filter=flt,
                                        view_weights=vw, **kw)
    assert np.array_equal(words(vol["weight"]), words(want["weight"]))
    assert np.array_equal(words(vol["tsdf"]), words(want["tsdf"]))
    mw = 0.5 * least_weight(float(fe["clean"].max()))
    mask, st = prior_from_depth_views(poses, intr, 48, 64, noisy, 4.0, depth_filter=flt,
                                      view_weights=vw, min_weight=mw, **kw)
    mask1, st1 = prior_from_depth_views(poses, intr, 48, 64, noisy, 4.0, depth_filter=flt, **kw)
    assert st["view_weights"]["kept"] == int((w > 0).sum()) and "view_weights" not in st1
    assert abs(st["observed"] - st1["observed"]) < 1e-6          # the same voxels were seen
    assert 0 < int(mask.sum()) < mask.numel()
    lab = np.full((16, 48, 64), 3, np.uint8)
    sem = fuse_semantic_views(poses, intr, 48, 64, noisy, lab, num_classes=5, depth_filter=flt,
                              view_weights=vw, **kw)
    sem1 = fuse_semantic_views(poses, intr, 48, 64, noisy, lab, num_classes=5, depth_filter=flt,
                               **kw)
    assert np.array_equal(words(sem["volume"]["weight"]), words(want["weight"]))
    assert torch.equal(sem["votes"], sem1["votes"]) and "view_weights" in sem
    # tracking without refinement (every frame is warm-up): one view per call
    tv = ops.tsdf_volume(dims, origin, float(h))
    ws = U.new_weight_stats()
    track_depth_views(tv, poses, intr, 48, 64, noisy, float(trunc), refine_warmup=16,
                      depth_filter=flt, view_weights=vw, view_weight_stats=ws)
    assert np.array_equal(words(tv["weight"]), words(want["weight"]))
    assert np.array_equal(words(tv["tsdf"]), words(want["tsdf"])) and ws["kept"] > 0
    for fn in (lambda: volume_from_depth_views(poses, intr, 48, 64, noisy, view_weights=vw, **kw),
               lambda: fuse_semantic_views(poses, intr, 48, 64, noisy, lab, view_weights=vw, **kw),
               lambda: track_depth_views(tv, poses, intr, 48, 64, noisy, float(trunc),
                                         view_weights=vw)):
        with pytest.raises(ValueError):
            fn()


def test_the_script_prints_its_line_and_is_unchanged_without_the_flag(tmp_path, capsys):
    """fuse_tsdf_mesh.py on an exported scene: with --view_weights it prints the
    view_weights: line; without it the PLY is, byte for byte, the one written
    from the restatement's unweighted volume of the front end's clean frames"""
    import os

    from PIL import Image

    from scripts import fuse_tsdf_mesh
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.mesh_render import read_frames
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    H, W, n = 48, 64, 8
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=H, W=W)
    h = room_volume_spec(48)[2]
    box = ["--voxel", repr(float(h)), "--aabb"] + [repr(v) for v in BOX] + ["--no_color"]
    out = str(tmp_path / "plain.ply")
    fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", out, "--depth_filter", "default"] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    assert not [l for l in lines if l.startswith("view_weights:")]
    out_w = str(tmp_path / "weighted.ply")
    rec = fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", out_w, "--depth_filter", "default",
                               "--view_weights", "default", "--min_weight", "0.05"] + box)
    lines = capsys.readouterr().out.strip().splitlines()
    line = [l for l in lines if l.startswith("view_weights: mean weight ")]
    assert len(line) == 1 and rec["vertices"] > 0
    mean = float(line[0].split()[3])
    assert 0.1 <= mean <= 1.0          # sigma_z2 = 0 by default: the clamped cosine alone
    assert open(out_w, "rb").read() != open(out, "rb").read()
    with pytest.raises(SystemExit):
        fuse_tsdf_mesh.main(["--scene_root", sroot, "--out", out_w, "--view_weights", "default"]
                            + box)
    # the unflagged run against the restatements
    fr = read_frames(sroot)
    uom = fr["one_m_to_scene_uom"]
    depth = np.stack([(np.asarray(Image.open(os.path.join(sroot, "depth", s + ".png")))
                       .astype(F32) / F32(1000.0)) * F32(uom) for s in fr["stems"]])
    from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter
    flt = DepthFilter().scaled(uom)
    fe = DN.frontend_vec(depth, DN.bilateral_tables(flt.radius, flt.sigma_space),
                         fr["intrinsics"], flt.sigma_depth, flt.max_jump, sigma_z2=flt.sigma_z2,
                         max_jump_z2=flt.max_jump_z2, min_cos=flt.min_cos, reject=flt.reject)
    # the lattice is the script's own choice: read it off its record
    vol = TN.new_volume(rec["dims"], rec["origin"], rec["voxel"])
    TN.integrate(vol, fe["clean"], fr["poses"], fr["intrinsics"], 4.0 * rec["voxel"])
    v, f, nrm = TN.extract(vol, 1.0)
    ref = str(tmp_path / "ref.ply")
    write_ply(ref, v, f, normals=nrm, rgb=None)
    assert open(out, "rb").read() == open(ref, "rb").read()
