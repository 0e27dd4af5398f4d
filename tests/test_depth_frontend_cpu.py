"""CPU-only: the depth front end's contracts as tests/depth_numpy.py restates
them (properties a filter and a normal map must have), the sensor model of
utils/depth_frontend.py, the settings object, and the wiring: header, library
and ctypes table agree on the three symbols and ``depth_filter=None`` reaches
none of the new code.  No kernel is launched."""
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import depth_numpy as DN

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ucsa_depth_filter", "ucsa_depth_normals", "ucsa_depth_frontend")
SETTINGS = ((2, 1.0), (3, 1.5), (4, 2.0))


def _utils():
    from ucsa_neural_rendering_amd.utils import depth_frontend
    return depth_frontend


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_frames(seed, B, H, W):
    """noisy two-level frames with every kind of pixel that is not a measurement"""
    g = np.random.default_rng(seed)
    z = (2.0 + 0.05 * g.standard_normal((B, H, W))).astype(F32)
    z[:, :, W // 2:] += F32(0.8)
    bad = g.random((B, H, W)) < 0.08
    z[bad] = g.choice(np.array([0.0, -1.0, np.nan, np.inf, -np.inf], F32), int(bad.sum()))
    return z


# ---------------------------------------------------------------------------
# the restatement: loops and arrays are one contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_the_array_form_has_the_loops_bytes(radius):
    z = random_frames(radius, 2, 11, 14)
    tb = DN.bilateral_tables(radius, 0.6 * radius)
    K = (13.0, 12.5, 7.3, 5.1)
    kw = dict(sigma_z2=0.004, max_jump_z2=0.002, min_cos=0.95, depth_min=0.5, depth_max=3.5)
    a = DN.frontend(z, tb, K, 0.05, 0.08, **kw)
    b = DN.frontend_vec(z, tb, K, 0.05, 0.08, **kw)
    for k in a:
        assert same(a[k], b[k]), k
    m = a["mask"]
    assert all(((m & bit) != 0).any() for bit in (1, 2, 4, 8)) and (m == 0).any()
    assert ((m & 2) == 0)[(m & 8) != 0].sum() == 0    # grazing needs a normal
    assert (a["clean"][(m & 12) != 0] == 0).all()
    keep = (m & 12) == 0
    assert same(a["clean"][keep], a["depth"][keep])


def test_tables_are_the_ops_tables():
    from ucsa_neural_rendering_amd.ops import depth as OD
    for r, s in SETTINGS:
        a, b = OD.bilateral_tables(r, s), DN.bilateral_tables(r, s)
        assert a["radius"] == r and same(a["w_space"], b["w_space"])
        assert same(a["w_range"], b["w_range"])
        assert a["w_space"].shape == ((2 * r + 1) ** 2,) and a["w_range"].shape == (256,)
        assert a["w_space"][len(a["w_space"]) // 2] == 1.0
        q = np.arange(256) + 0.5
        assert np.allclose(a["w_range"], np.exp(-0.5 * (q * 3 / 256) ** 2), rtol=1e-7, atol=0)
    with pytest.raises(OD._lib.UcsaError):
        OD.bilateral_tables(5, 1.0)
    with pytest.raises(OD._lib.UcsaError):
        OD.bilateral_tables(2, 1.0, Q=128)


# ---------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", [DN.filter, DN.filter_vec])
def test_a_constant_image_comes_back_with_its_own_bits(form):
    z = np.full((1, 9, 12), 2.3456789, F32)
    for r, s in SETTINGS + ((1, 0.5),):
        assert same(form(z, DN.bilateral_tables(r, s), 0.01, 0.003), z)


@pytest.mark.parametrize("form", [DN.filter, DN.filter_vec])
def test_a_step_edge_is_not_blurred_and_holes_stay_holes(form):
    z = np.full((1, 10, 12), 1.5, F32)
    z[:, :, 6:] = 2.5
    z[0, 4, 5] = 0.0
    z[0, 5, 6] = np.nan
    out = form(z, DN.bilateral_tables(3, 1.5), 0.01)
    want = z.copy()
    want[0, 5, 6] = 0.0
    assert same(out, want)


def test_noise_on_a_plane_falls_as_a_linear_filter_would_reduce_it():
    """A fronto-parallel plane at z = 2 with Gaussian noise sigma = 0.01, 64 x 80,
    sigma_depth = 5 sigma: every neighbour takes part and the range weight is
    nearly flat, so the filter is close to the linear filter with the space
    table, whose rms ratio for white noise is sqrt(sum w^2) / sum w.  Bound:
    1.25 times that.  Measured here for (r, sigma_s) = (2, 1), (3, 1.5), (4, 2):
    0.3123 / 0.2170 / 0.1687 against 0.2873 / 0.1947 / 0.1476 (the range
    weight is not quite flat: (d / sigma_depth)^2 averages 2 / 25, which keeps a
    pixel about 8 % closer to its own noise)."""
    g = np.random.default_rng(5)
    noise = (0.01 * g.standard_normal((1, 64, 80)))
    z = (2.0 + noise).astype(F32)
    for r, s in SETTINGS:
        tb = DN.bilateral_tables(r, s)
        out = DN.filter_vec(z, tb, 0.05)
        inner = (slice(None), slice(r, -r), slice(r, -r))
        ratio = float(np.sqrt(np.mean((out[inner].astype(np.float64) - 2.0) ** 2))
                      / np.sqrt(np.mean((z[inner].astype(np.float64) - 2.0) ** 2)))
        w = tb["w_space"].astype(np.float64)
        ideal = math.sqrt((w ** 2).sum()) / w.sum()
        print(f"r {r} sigma_s {s}: rms ratio {ratio:.4f}, linear filter {ideal:.4f}")
        assert ratio <= 1.25 * ideal


# ---------------------------------------------------------------------------
# points and normals
# ---------------------------------------------------------------------------
def test_points_of_an_unfiltered_frame_are_backprojects_bytes():
    from ucsa_neural_rendering_amd.utils.registration import backproject
    z = random_frames(2, 1, 37, 45)
    K = (41.7, 39.2, 20.9, 17.3)          # an off-centre principal point
    points, _, mask = DN.normals(z, K, 0.1, depth_min=1e-6, depth_max=3.0e38)
    got = points[(mask & 1) != 0]
    want = backproject(torch.from_numpy(z[0]), K, 1, 1e-6, 3.0e38).numpy()
    assert want.shape[0] > 1000 and same(got, want)
    pv, _, mv = DN.normals_vec(z, K, 0.1)
    assert same(pv, points) and same(mv, mask)


def test_normals_of_a_tilted_plane_are_the_planes_normal():
    """The plane n . X = c seen by a pinhole camera: z(i, j) = c / (n . ray(i, j))
    in float64, rounded to float32.  The back-projected points lie on the plane
    up to rounding, so every difference of two of them lies in it and dv x du
    is the plane's normal, whichever of the three differences a pixel takes.
    The bound, first order in eps = 2^-24: a coordinate of a point carries at
    most four roundings (z's, and for x or y the subtraction, the division and
    the product), so a point is off by delta <= 4 sqrt(3) eps max|P|; a
    difference of two points by 2 delta, which turns a tangent of length >= s
    (the least one-pixel step on the plane) by 2 delta / s; two tangents that
    meet at an angle theta turn their cross product by at most the sum of the
    two over sin(theta); the differences, the cross product, the normalisation
    add a few eps of their own (16 eps allowed).  Here: bound 1.9e-4 rad,
    measured 4.1e-6 rad."""
    H, W = 40, 52
    K = (48.0, 47.0, 25.2, 19.4)
    n = np.array([0.35, -0.25, -0.9])
    n /= np.linalg.norm(n)
    c = float(n @ np.array([0.0, 0.0, 2.0]))
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.stack([(jj + 0.5 - K[2]) / K[0], (ii + 0.5 - K[3]) / K[1], np.ones((H, W))], -1)
    z64 = c / (ray @ n)
    assert z64.min() > 1.0
    P = ray * z64[..., None]
    points, nrm, mask = DN.normals(z64[None].astype(F32), K, 1.0)
    assert (mask == 3).all()
    eps = 2.0 ** -24
    delta = 4.0 * math.sqrt(3.0) * eps * np.abs(P).max()
    du, dv = P[:, 1:] - P[:, :-1], P[1:] - P[:-1]
    s = min(np.linalg.norm(du, axis=-1).min(), np.linalg.norm(dv, axis=-1).min())
    a, b = du[:-1], dv[:, :-1]
    sin_uv = (np.linalg.norm(np.cross(a, b), axis=-1)
              / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))).min()
    bound = 2.0 * (2.0 * delta / s) / sin_uv + 16.0 * eps
    want = n if n @ P[0, 0] < 0 else -n                  # towards the camera
    got = nrm[0].astype(np.float64)
    angle = np.arctan2(np.linalg.norm(np.cross(got, want), axis=-1), got @ want)
    print(f"tilted plane: largest angle {angle.max():.3e} rad, bound {bound:.3e} rad")
    assert abs(np.linalg.norm(got, axis=-1) - 1.0).max() < 4 * eps
    assert angle.max() <= bound
    assert np.abs(points[0] - P).max() <= delta


def test_edges_jumps_and_grazing_bits():
    z = np.full((1, 7, 9), 2.0, F32)
    z[0, :, 5:] = F32(2.0) + F32(0.25)      # a jump of exactly max_jump: still usable
    _, nrm, mask = DN.normals(z, (10.0, 10.0, 4.5, 3.5), 0.25)
    assert (mask == 3).all()
    z[0, :, 5:] = np.nextafter(F32(2.25), F32(3))
    _, nrm, mask = DN.normals(z, (10.0, 10.0, 4.5, 3.5), 0.25)
    assert (mask[0, :, 4:6] == 7).all() and (mask[0, :, :4] == 3).all()
    assert (mask[0, :, 6:] == 3).all()
    assert np.allclose(nrm[0], [0, 0, -1], atol=1e-6)   # one-sided differences at the edge
    # an isolated pixel has no usable neighbour: no normal
    z[0, 3, 2] = 5.0
    _, nrm, mask = DN.normals(z, (10.0, 10.0, 4.5, 3.5), 0.25)
    assert mask[0, 3, 2] == 5 and not nrm[0, 3, 2].any()
    # a wall seen at about 80 degrees from its normal: cos = 0.17
    # (z = 2 + tan(80 deg) x with x = a z, a within +-0.04: cos between 0.13 and 0.21)
    a = (np.arange(9) + 0.5 - 4.5) / 100.0
    wall = (2.0 / (1.0 - math.tan(math.radians(80)) * a))[None, None, :].repeat(7, 1)
    for min_cos, bits in ((0.1, 3), (0.9, 11)):
        _, _, mask = DN.normals(wall.astype(F32), (100.0, 100.0, 4.5, 3.5), 1.0, min_cos=min_cos)
        assert (mask == bits).all(), (min_cos, np.unique(mask))


# ---------------------------------------------------------------------------
# the sensor model and the settings
# ---------------------------------------------------------------------------
def test_sensor_model_is_deterministic_and_does_what_it_says():
    U = _utils()
    z = np.full((2, 20, 24), 2.0)
    z[:, :, 12:] = 3.0
    z[0, 3, 3] = 0.0
    kw = dict(sigma0=0.002, sigma_z2=0.001, quantum=0.001, flying_share=0.5, jump=0.3)
    a, fa = U.simulate_sensor_noise(z, 7, return_flying=True, **kw)
    b = U.simulate_sensor_noise(z, 7, **kw)
    assert a.dtype == np.float32 and same(a, b)
    assert not same(a, U.simulate_sensor_noise(z, 8, **kw))
    assert a[0, 3, 3] == 0.0
    assert np.abs(a / 0.001 - np.round(a / 0.001)).max() < 1e-3          # quantised
    assert fa[:, :, 11:13].mean() > 0.3 and not fa[:, :, :11].any() and not fa[:, :, 13:].any()
    assert ((a[fa] > 1.95) & (a[fa] < 3.05)).all() and ((a[fa] > 2.1) & (a[fa] < 2.9)).any()
    flat = ~fa & (z > 0)
    flat[:, :, 11:13] = False
    err = a[flat] - z[flat]
    assert 0.004 < err[z[flat] == 2.0].std() < 0.008      # 0.002 + 0.001 * 4
    assert 0.008 < err[z[flat] == 3.0].std() < 0.014      # 0.002 + 0.001 * 9
    assert same(U.simulate_sensor_noise(z, 1), np.where(z > 0, z, 0).astype(F32))


def test_settings_from_string():
    U = _utils()
    d = U.DepthFilter()
    assert U.DepthFilter.from_string("default") == d == U.DepthFilter.from_string("")
    f = U.DepthFilter.from_string("radius=3, sigma_space=1.5,sigma_depth=0.02,reject_grazing=0")
    assert (f.radius, f.sigma_space, f.sigma_depth, f.reject_grazing) == (3, 1.5, 0.02, False)
    assert isinstance(f.radius, int) and f.reject == 4 and d.reject == 12
    assert dataclass_replace(d, reject_edges=False).reject == 8
    s = U.DepthFilter(sigma_depth=0.01, sigma_z2=0.002, max_jump=0.05, max_jump_z2=0.004).scaled(2)
    assert (s.sigma_depth, s.sigma_z2, s.max_jump, s.max_jump_z2) == (0.02, 0.001, 0.1, 0.002)
    for bad in ("radius", "colour=1", "reject_edges=maybe"):
        with pytest.raises(ValueError):
            U.DepthFilter.from_string(bad)


def dataclass_replace(obj, **kw):
    import dataclasses
    return dataclasses.replace(obj, **kw)


def test_sensed_room_views_lose_their_flying_pixels_and_little_else():
    """Six views of SyntheticRoom(0) at 120 x 160 through simulate_sensor_noise
    (sigma 0.001 + 0.0005 z^2, quantum 0.001, half of the pixels whose 3 x 3
    neighbourhood spans more than 0.3 fly), then the front end with r = 2,
    sigma_depth 0.01 + 0.003 z^2, max_jump 0.05 + 0.01 z^2 (the room is seen
    from 3.5 to 6.3 units away, where a pixel on a slanted wall steps by up to
    0.2).  The edge bit must remove at least as many flying pixels as it leaves:
    measured 55 removed, 6 left.  The share of the measured pixels that do not
    fly and are rejected all the same: a flying pixel sits within one pixel of a
    discontinuity of the exact frame, so what it can spoil lies within two
    pixels of one, and the exact frame's own edge pixels are those within one
    pixel; the cap is twice the exact frame's share.  Measured 0.00121 against a
    cap of 0.00243."""
    from tests.test_tsdf_fusion_cpu import room_frames
    U = _utils()
    _, _, intr, depth = room_frames(120, 160, 6)
    noisy, fly = U.simulate_sensor_noise(depth, 3, 0.001, 0.0005, 0.001, 0.5, 0.3,
                                         return_flying=True)
    tb = DN.bilateral_tables(2, 1.0)
    args = (tb, intr, 0.01, 0.05)
    kw = dict(sigma_z2=0.003, max_jump_z2=0.01, min_cos=0.1)
    exact = DN.frontend_vec(depth, *args, **kw)
    sensed = DN.frontend_vec(noisy, *args, **kw)
    cap = 2.0 * float(((exact["mask"] & 12) != 0).mean())
    rejected = (sensed["mask"] & 12) != 0
    measured = (sensed["mask"] & 1) != 0
    removed, left = int((fly & rejected).sum()), int((fly & ~rejected).sum())
    share = float((rejected & ~fly & measured).sum() / (measured & ~fly).sum())
    print(f"flying {int(fly.sum())}: removed {removed}, left {left}; others rejected "
          f"{share:.5f}, cap {cap:.5f}")
    assert fly.sum() >= 40 and removed >= left
    assert share <= cap
    assert float(((exact["mask"] & 12) != 0).mean()) <= cap
    assert (sensed["clean"][rejected] == 0).all()


# ---------------------------------------------------------------------------
# symbols and wiring
# ---------------------------------------------------------------------------
def test_header_library_and_table_agree_on_the_three_symbols():
    from ucsa_neural_rendering_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ucsa_hip.h")).read(),
                    flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    for name in SYMBOLS:
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, header)
        assert decl, name
        assert re.search(r" T %s$" % name, nm, re.M), name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == decl.group(1).count(",") + 1, name
    l = _lib.lib()
    # an argument error names its index and nothing is launched (there is no GPU here)
    assert l.ucsa_depth_filter(None, 1, 1, 1, None, 1, None, 1.0, 0.0, 0.0, 1.0, None, None) == -1000
    one = torch.zeros(4).data_ptr()
    assert l.ucsa_depth_filter(one, 1, 1, 1, one, 5, one, 1.0, 0.0, 0.0, 1.0, one, None) == -1005
    assert l.ucsa_depth_normals(one, 1, 1, 1, 0.0, 1.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 1.0,
                                one, one, one, None) == -1004
    assert l.ucsa_depth_frontend(one, 1, 1, 1, one, 1, one, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.1,
                                 0.0, 0.0, 16, 0.0, 1.0, one, one, one, one, one, None) == -1016


def test_cpu_tensors_are_refused_before_the_library_is_reached(monkeypatch):
    from ucsa_neural_rendering_amd import _lib, ops

    def no_lib():
        raise AssertionError("lib() reached")
    monkeypatch.setattr(ops.depth, "lib", no_lib)
    z = torch.ones(1, 4, 4)
    tb = ops.depth.bilateral_tables(1, 1.0)
    with pytest.raises(_lib.UcsaError):
        ops.depth.filter_depth(z, tb, 0.01)
    with pytest.raises(_lib.UcsaError):
        ops.depth.depth_normals(z, (4.0, 4.0, 2.0, 2.0), 0.1)
    with pytest.raises(_lib.UcsaError):
        ops.depth.depth_frontend(z, tb, (4.0, 4.0, 2.0, 2.0), 0.01, 0.1)
    with pytest.raises(_lib.UcsaError):
        ops.depth.filter_depth(z.numpy(), tb, 0.01)
    surface = json_surface()                  # the flat surface of ops stays frozen
    assert not [n for n in ("filter_depth", "depth_normals", "depth_frontend") if n in surface]
    assert not hasattr(ops, "filter_depth") and not hasattr(ops, "depth_frontend")


def json_surface():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "ops_api.json")) as f:
        return json.dumps(json.load(f))


def test_depth_filter_none_reaches_none_of_the_new_code(monkeypatch):
    """Every consumer has ``depth_filter=None``; with None the tracking entry
    points hand ``backproject``'s points on unchanged and the front end's module
    is never asked for anything."""
    from ucsa_neural_rendering_amd.utils import (depth_frontend, occupancy_prior, registration,
                                                 tsdf_fusion, voxel_map)
    for fn in (tsdf_fusion.fuse_depth_views, tsdf_fusion.track_depth_views,
               registration.refine_pose_tsdf, registration.refine_pose,
               occupancy_prior.prior_from_depth_views, voxel_map.fuse_semantic_views):
        assert inspect.signature(fn).parameters["depth_filter"].default is None, fn.__name__
    for name in ("run_frontend", "clean_depth", "frame_points", "new_stats", "_tables"):
        monkeypatch.setattr(depth_frontend, name,
                            lambda *a, **k: pytest.fail("the front end was entered"))
    seen = {}

    def fake_register(points, *a, **k):
        seen["points"] = points
        return {"transform": np.eye(4)}
    monkeypatch.setattr(registration, "register_points", fake_register)
    monkeypatch.setattr(registration, "register_points_tsdf", fake_register)
    z = torch.from_numpy(random_frames(4, 1, 12, 16)[0])
    K = (14.0, 14.0, 8.0, 6.0)
    want = registration.backproject(z, K, 2)
    registration.refine_pose(z, np.eye(4), K, {"verts": None, "faces": None}, stride=2,
                             device="cpu")
    assert torch.equal(seen.pop("points"), want)
    registration.refine_pose_tsdf(z, np.eye(4), K, None, 0.1, stride=2, device="cpu")
    assert torch.equal(seen.pop("points"), want)
    # the other four enter the front end only under `depth_filter is not None`
    for mod in (tsdf_fusion, occupancy_prior, voxel_map):
        src = inspect.getsource(mod)
        for m in re.finditer(r"^( *)([^`\n]*depth_frontend\.\w+\(.*)$", src, re.M):
            head = src[:m.start()].rstrip().splitlines()
            guard = [l for l in head if l.strip().startswith("if depth_filter is not None")][-1]
            assert len(guard) - len(guard.lstrip()) < len(m.group(1)), m.group(2)
