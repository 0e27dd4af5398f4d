"""GPU: the depth front end (csrc/depth_frontend.hip) against the numpy
restatement of its contracts (tests/depth_numpy.py, the plain loops): every
output of ucsa_depth_filter, ucsa_depth_normals and ucsa_depth_frontend as
int32 / uint8 words; the fused launch against the two launches; two runs; the
input untouched; guard words; argument codes; and the front end inside the
fusion, end to end, on sensed views of the synthetic room."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import depth_numpy as DN

pytestmark = pytest.mark.gpu

F32 = np.float32
K_OFF = (23.7, 22.1, 11.3, 6.2)      # an off-centre principal point
OUTPUTS = ("depth", "clean", "points", "normals", "mask")


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.uint8)


def frames(seed, B, H, W, dmin, dmax):
    """two noisy levels, a ramp, every kind of pixel that is no measurement, and
    pixels exactly at and just outside depth_min and depth_max"""
    g = np.random.default_rng(seed)
    z = (2.0 + 0.04 * g.standard_normal((B, H, W))).astype(F32)
    z[:, :, W // 2:] += F32(0.5)
    z += (0.02 * np.arange(H, dtype=F32))[None, :, None]
    special = [0.0, -1.5, np.nan, np.inf, -np.inf, dmin, np.nextafter(F32(dmin), F32(0))]
    if dmax < 1e30:
        special += [dmax, np.nextafter(F32(dmax), F32(9))]
    special = np.array(special, F32)
    pick = g.random((B, H, W)) < 0.15
    z[pick] = g.choice(special, int(pick.sum()))
    return z


def run_gpu(z, tables, K, sigma_depth, max_jump, **kw):
    """the three entry points; asserts what must hold between them -> the fused dict"""
    ops = _ops()
    d = _cu(z)
    before = d.clone()
    fkw = {k: kw[k] for k in ("sigma_z2", "depth_min", "depth_max") if k in kw}
    nkw = {k: kw[k] for k in ("max_jump_z2", "min_cos", "depth_min", "depth_max") if k in kw}
    f = ops.depth.filter_depth(d, tables, sigma_depth, **fkw)
    n = ops.depth.depth_normals(f, K, max_jump, **nkw)
    fused = ops.depth.depth_frontend(d, tables, K, sigma_depth, max_jump, **kw)
    again = ops.depth.depth_frontend(d, tables, K, sigma_depth, max_jump, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(words(d), words(before)), "the input was written"
    assert np.array_equal(words(fused["depth"]), words(f))
    for k in ("points", "normals", "mask"):
        assert np.array_equal(words(fused[k]), words(n[k])), k
    for k in OUTPUTS:
        assert np.array_equal(words(fused[k]), words(again[k])), k
    return {k: fused[k].cpu().numpy() for k in OUTPUTS}


def check(z, radius, K, sigma_depth, max_jump, **kw):
    tables = DN.bilateral_tables(radius, 0.5 * radius + 0.25)
    want = DN.frontend(z, tables, K, sigma_depth, max_jump, **kw)
    got = run_gpu(z, tables, K, sigma_depth, max_jump, **kw)
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert np.array_equal(words(got[k]), words(want[k])), (k, radius, z.shape)
    return want


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 2), (1, 16, 16), (3, 17, 33), (1, 13, 50)])
def test_every_output_is_the_restatements_words(shape):
    """1 x 1; a window larger than the image; one tile exactly; tiles with a
    ragged edge in both directions; B = 1 and 3; r = 1..4"""
    dmin, dmax = 1.25, 3.0
    z = frames(sum(shape), *shape, dmin, dmax)
    seen = np.zeros(16, bool)
    for radius in (4,) if shape == (1, 3, 2) else (1, 2, 3, 4):
        want = check(z, radius, K_OFF, 0.05, 0.09, sigma_z2=0.004, max_jump_z2=0.003,
                     min_cos=0.93, reject=12, depth_min=dmin, depth_max=dmax)
        seen[np.unique(want["mask"])] = True
    if shape[1] >= 13:
        assert seen[[0, 1, 3, 5, 7, 11, 15]].all(), np.flatnonzero(seen)


def test_reject_sets_and_default_range():
    z = frames(9, 2, 17, 33, 1e-6, 3.0e38)
    for reject in (0, 4, 8):
        want = check(z, 2, K_OFF, 0.05, 0.09, max_jump_z2=0.003, min_cos=0.93, reject=reject)
        gone = (want["mask"] & reject) != 0
        assert (want["clean"][gone] == 0).all()
        assert np.array_equal(words(want["clean"][~gone]), words(want["depth"][~gone]))


def test_a_frame_without_a_measurement_gives_zeros():
    z = np.zeros((2, 17, 20), F32)
    z[1] = np.nan
    z[0, 3, 3], z[0, 4, 4], z[1, 5, 5] = -2.0, np.inf, 9.0      # 9 > depth_max
    want = check(z, 3, K_OFF, 0.05, 0.1, depth_min=1e-6, depth_max=8.0)
    for k in OUTPUTS:
        assert not words(want[k]).any(), k


def test_the_range_gate_at_exactly_three_sigma():
    """sigma_depth = float32(1/3): 3 sigma rounds to 1, scale is 256 and a
    neighbour 1 away sits at t = Q exactly (out), one float32 step nearer at
    t < Q (in, bin 255)"""
    s = float(F32(1.0 / 3.0))
    assert F32(3.0) * F32(s) == F32(1.0)
    z = np.full((1, 5, 7), 2.0, F32)
    z[0, 2, 3] = 3.0
    at = check(z, 1, K_OFF, s, 10.0)
    assert np.array_equal(words(at["depth"]), words(z))          # t = Q: took no part
    z[0, 2, 3] = np.nextafter(F32(3.0), F32(0))
    below = check(z, 1, K_OFF, s, 10.0)
    assert below["depth"][0, 2, 2] > 2.0 and below["depth"][0, 2, 3] < z[0, 2, 3]


def test_jumps_at_exactly_max_jump_and_a_grazing_wall():
    K = (10.0, 10.0, 4.5, 3.5)
    z = np.full((1, 7, 9), 2.0, F32)
    z[0, :, 5:] = 2.25
    want = check(z, 1, K, 0.001, 0.25)
    assert (want["mask"] == 3).all()
    z[0, :, 5:] = np.nextafter(F32(2.25), F32(3))
    want = check(z, 1, K, 0.001, 0.25)
    assert (want["mask"][0, :, 4:6] == 7).all() and (want["mask"][0, :, :4] == 3).all()
    assert not want["clean"][0, :, 4:6].any()
    a = (np.arange(9) + 0.5 - 4.5) / 100.0
    wall = (2.0 / (1.0 - np.tan(np.radians(80.0)) * a))[None, None, :].repeat(7, 1).astype(F32)
    for min_cos, bits in ((0.1, 3), (0.9, 11)):
        want = check(wall, 1, (100.0, 100.0, 4.5, 3.5), 0.001, 1.0, min_cos=min_cos)
        assert (want["mask"] == bits).all()


def test_nothing_is_written_outside_the_outputs():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd.ops._args import _stream
    B, H, W, G = 3, 17, 33, 1024
    z = frames(4, B, H, W, 1e-6, 3.0e38)
    tb = DN.bilateral_tables(4, 2.0)
    want = DN.frontend(z, tb, K_OFF, 0.05, 0.09, min_cos=0.9)
    d, ws, wr = _cu(z), _cu(tb["w_space"]), _cu(tb["w_range"])
    n = B * H * W
    bufs = {k: torch.full((2 * G + n * per,), -777.25 if dt == torch.float32 else 0xA5,
                          dtype=dt, device="cuda")
            for k, per, dt in (("depth", 1, torch.float32), ("clean", 1, torch.float32),
                               ("points", 3, torch.float32), ("normals", 3, torch.float32),
                               ("mask", 1, torch.uint8))}
    ptr = {k: C.c_void_p(b.data_ptr() + G * b.element_size()) for k, b in bufs.items()}
    rc = _lib.lib().ucsa_depth_frontend(
        C.c_void_p(d.data_ptr()), B, H, W, C.c_void_p(ws.data_ptr()), 4,
        C.c_void_p(wr.data_ptr()), 0.05, 0.0, *K_OFF, 0.09, 0.0, 0.9, 12, 1e-6, 3.0e38,
        ptr["depth"], ptr["clean"], ptr["points"], ptr["normals"], ptr["mask"], _stream())
    torch.cuda.synchronize()
    assert rc == 0
    for k, b in bufs.items():
        guard = b[:G].cpu().numpy(), b[-G:].cpu().numpy()
        fill = b.new_full((G,), -777.25 if b.dtype == torch.float32 else 0xA5).cpu().numpy()
        assert np.array_equal(guard[0], fill) and np.array_equal(guard[1], fill), k
        assert np.array_equal(words(b[G:-G]).reshape(-1), words(want[k]).reshape(-1)), k


def test_one_argument_error_per_limit_and_no_launch():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    z = _cu(np.full((1, 4, 4), 2.0, F32))
    tb = DN.bilateral_tables(1, 1.0)
    ws, wr = _cu(tb["w_space"]), _cu(tb["w_range"])
    out = {k: torch.full((48,), 7, dtype=torch.uint8 if k == "mask" else torch.float32,
                         device="cuda") for k in OUTPUTS}
    p = lambda t: C.c_void_p(t.data_ptr())
    good_f = [p(z), 1, 4, 4, p(ws), 1, p(wr), 0.01, 0.0, 1e-6, 3.0e38, p(out["depth"]), None]
    good_n = [p(z), 1, 4, 4, 4.0, 4.0, 2.0, 2.0, 0.1, 0.0, 0.0, 1e-6, 3.0e38, p(out["points"]),
              p(out["normals"]), p(out["mask"]), None]
    good_x = [p(z), 1, 4, 4, p(ws), 1, p(wr), 0.01, 0.0, 4.0, 4.0, 2.0, 2.0, 0.1, 0.0, 0.0, 12,
              1e-6, 3.0e38, p(out["depth"]), p(out["clean"]), p(out["points"]),
              p(out["normals"]), p(out["mask"]), None]
    nan = float("nan")
    cases = [
        (l.ucsa_depth_filter, good_f, [(1, 0), (2, 0), (2, 16385), (3, 0), (3, 16385), (5, 0),
                                       (5, 5), (7, 0.0), (7, nan), (8, -1.0), (9, nan),
                                       (10, 0.0), (11, None), (0, None), (4, None), (6, None)]),
        (l.ucsa_depth_normals, good_n, [(1, 0), (2, 16385), (3, 0), (4, 0.0), (5, -1.0),
                                        (6, nan), (7, nan), (8, -0.1), (9, -0.1), (10, 1.5),
                                        (10, -1.5), (11, nan), (12, 0.0), (13, None),
                                        (14, None), (15, None)]),
        (l.ucsa_depth_frontend, good_x, [(1, 0), (2, 0), (3, 16385), (5, 0), (5, 5), (7, 0.0),
                                         (8, -1.0), (9, 0.0), (10, 0.0), (11, nan), (12, nan),
                                         (13, -0.1), (14, -0.1), (15, 1.5), (16, 1), (16, 16),
                                         (17, nan), (18, 0.0), (19, None), (20, None),
                                         (21, None), (22, None), (23, None)]),
    ]
    for fn, good, bad in cases:
        for k, v in bad:
            args = list(good)
            args[k] = v
            assert fn(*args) == -1000 - k, (fn.__name__, k, v)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert (t == 7).all(), k            # nothing was launched
    for fn, good, _ in cases:
        assert fn(*good) == 0
    # the wrappers refuse the same before the library is reached
    ops = _ops()
    for bad in (dict(sigma_depth=0.0), dict(max_jump=-1.0), dict(min_cos=2.0), dict(reject=3),
                dict(sigma_z2=-1.0), dict(max_jump_z2=-1.0), dict(intrinsics=(0.0, 4.0, 2.0, 2.0))):
        kw = dict(sigma_depth=0.01, max_jump=0.1, intrinsics=(4.0, 4.0, 2.0, 2.0))
        kw.update(bad)
        with pytest.raises(_lib.UcsaError):
            ops.depth.depth_frontend(z, tb, **kw)
    with pytest.raises(_lib.UcsaError):
        ops.depth.filter_depth(z.cpu(), tb, 0.01)


# ---------------------------------------------------------------------------
# inside the fusion
# ---------------------------------------------------------------------------
BOX = [-3.05] * 3 + [3.05] * 3


def test_sensed_room_views_fuse_closer_to_the_room_with_the_front_end():
    """16 views of SyntheticRoom(0) at 48 x 64 through simulate_sensor_noise
    (sigma 0.02 + 0.002 z^2, quantum 0.001, half of the pixels whose 3 x 3
    neighbourhood spans more than 0.3 fly), fused at 64^3 with and without
    DepthFilter(r = 3, sigma_space 1.5, sigma_depth 0.06 + 0.006 z^2, max_jump
    0.05 + 0.02 z^2, min_cos 0.1).  The yardstick is the unfiltered run on the
    same frames.  The numpy pipeline (restatement + tests/tsdf_numpy.py) gives a
    median vertex distance to the analytic room of 0.406 voxels without and
    0.094 with the front end (0.038 on the exact frames)."""
    from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec, vertex_distance_voxels
    from ucsa_neural_rendering_amd.utils.depth_frontend import (DepthFilter, clean_depth,
                                                                simulate_sensor_noise, stats_line)
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import fuse_depth_views
    room, poses, intr, depth = room_frames(48, 64, 16)
    dims, _, h, trunc = room_volume_spec(64)
    noisy = simulate_sensor_noise(depth, 3, 0.02, 0.002, 0.001, 0.5, 0.3)
    flt = DepthFilter(radius=3, sigma_space=1.5, sigma_depth=0.06, sigma_z2=0.006,
                      max_jump=0.05, max_jump_z2=0.02, min_cos=0.1)
    kw = dict(aabb=BOX, voxel=float(h), trunc=float(trunc))
    args = (poses, intr, 48, 64, noisy)
    raw = fuse_depth_views(*args, **kw)
    off = fuse_depth_views(*args, depth_filter=None, **kw)
    on = fuse_depth_views(*args, depth_filter=flt, **kw)
    assert raw["dims"] == on["dims"] == tuple(dims)
    assert "depth_filter" not in off
    for k in ("verts", "faces", "normals"):                       # off gives the former bytes
        assert raw[k].tobytes() == off[k].tobytes(), k
    # the fusion integrated exactly the front end's clean frames
    want = DN.frontend_vec(noisy, DN.bilateral_tables(3, 1.5), intr, 0.06, 0.05, sigma_z2=0.006,
                           max_jump_z2=0.02, min_cos=0.1)["clean"]
    assert np.array_equal(words(clean_depth(_cu(noisy), intr, flt)), words(want))
    st = on["depth_filter"]
    assert st["pixels"] == noisy.size and 0 < st["rejected"] < 0.05 * st["measured"]
    assert stats_line(st).startswith("depth_filter: ")
    med = {k: float(np.median(vertex_distance_voxels(room, m["verts"], h)))
           for k, m in (("raw", raw), ("filtered", on))}
    small = {}
    for k, f in (("raw", None), ("filtered", flt)):
        c = fuse_depth_views(*args, depth_filter=f, min_component=50, **kw)["components"]
        small[k] = c["removed_components"] / max(1, c["components"])
    print(f"median vertex distance to the room, voxels: raw {med['raw']:.4f}, with the front "
          f"end {med['filtered']:.4f}; share of components under 50 voxels: raw "
          f"{small['raw']:.4f}, with the front end {small['filtered']:.4f}; {stats_line(st)}")
    assert med["filtered"] < med["raw"]
    assert small["filtered"] <= small["raw"]


def test_tracking_takes_the_kept_pixels_points():
    from ucsa_neural_rendering_amd.utils import registration as REG
    from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter, frame_points
    z = frames(12, 1, 21, 30, 1e-6, 3.0e38)
    flt = DepthFilter(radius=2, sigma_space=1.0, sigma_depth=0.05, max_jump=0.09, min_cos=0.9)
    want = DN.frontend(z, DN.bilateral_tables(2, 1.0), K_OFF, 0.05, 0.09, min_cos=0.9)
    for stride in (1, 2):
        m = want["mask"][0, ::stride, ::stride]
        keep = ((m & 1) != 0) & ((m & 12) == 0)
        pts, nrm = frame_points(_cu(z[0]), K_OFF, flt, stride)
        assert 0 < keep.sum() < m.size
        assert np.array_equal(words(pts), words(want["points"][0, ::stride, ::stride][keep]))
        assert np.array_equal(words(nrm), words(want["normals"][0, ::stride, ::stride][keep]))
        got = REG._frame_points(_cu(z[0]), K_OFF, stride, 0.0, float("inf"), flt)
        assert np.array_equal(words(got), words(pts))


def test_the_launches_utils_picks_change_no_byte():
    from ucsa_neural_rendering_amd.utils import depth_frontend as U
    assert U.fused_is_faster(1, 4) and U.fused_is_faster(16, 2) and not U.fused_is_faster(16, 3)
    z = _cu(frames(21, 3, 17, 33, 1e-6, 3.0e38))
    for radius in (2, 3):                      # one launch; two launches
        flt = U.DepthFilter(radius=radius, sigma_space=1.0, sigma_depth=0.05, sigma_z2=0.004,
                            max_jump=0.09, max_jump_z2=0.003, min_cos=0.93, reject_grazing=False)
        got = U.run_frontend(z, K_OFF, flt)
        want = _ops().depth.depth_frontend(
            z, DN.bilateral_tables(radius, 1.0), K_OFF, 0.05, 0.09, sigma_z2=0.004,
            max_jump_z2=0.003, min_cos=0.93, reject=4)
        assert sorted(got) == sorted(want)
        for k in OUTPUTS:
            assert np.array_equal(words(got[k]), words(want[k])), (radius, k)


def test_the_three_scripts_take_a_depth_filter(tmp_path, capsys):
    """four exported 60 x 80 views: each script prints its one ``depth_filter:``
    line with the flag and none without it"""
    from scripts import fuse_tsdf_mesh, occupancy_prior, voxel_map_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    _, sroot = export(str(tmp_path), scene_seed=0, n_views=4, H=60, W=80)
    spec = "radius=2,sigma_depth=0.01,sigma_z2=0.003,max_jump=0.05,max_jump_z2=0.02"
    box = ["--aabb", "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05"]
    runs = (
        (fuse_tsdf_mesh, ["--scene_root", sroot, "--out", str(tmp_path / "m.ply"), "--voxel",
                          "0.1", "--no_color"] + box),
        (voxel_map_labels, ["--scene_root", sroot, "--labels", "label_40", "--out_dir",
                            str(tmp_path / "vm"), "--voxel", "0.1"] + box),
        (occupancy_prior, ["--scene_root", sroot, "--out", str(tmp_path / "p.npz"), "--voxel",
                           "0.1"]),
    )
    for script, argv in runs:
        script.main(argv)
        assert "depth_filter:" not in capsys.readouterr().out, script.__name__
        script.main(argv + ["--depth_filter", spec])
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("depth_filter:")]
        assert len(lines) == 1 and "edge (bit 4)" in lines[0], script.__name__
        assert f"of {4 * 60 * 80} pixels" in lines[0], lines[0]
    with pytest.raises(ValueError):
        fuse_tsdf_mesh.main(runs[0][1] + ["--depth_filter", "radius"])


def test_tracking_while_fusing_goes_through_the_front_end():
    """fuse_depth_views(refine_poses=True, depth_filter=...): every frame is
    tracked with the kept pixels' points and integrated with its clean depth;
    at the true poses the tracker must leave them within its own step limits"""
    from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec
    from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import fuse_depth_views
    _, poses, intr, depth = room_frames(48, 64, 6)
    _, _, h, trunc = room_volume_spec(64)
    flt = DepthFilter(radius=2, sigma_space=1.0, sigma_depth=0.01, sigma_z2=0.003,
                      max_jump=0.05, max_jump_z2=0.02, min_cos=0.1)
    out = fuse_depth_views(poses, intr, 48, 64, depth, aabb=BOX, voxel=float(h),
                           trunc=float(trunc), refine_poses=True, depth_filter=flt,
                           refine_kw={"iterations": 5, "stride": 2})
    assert out["poses"].shape == (6, 4, 4) and out["refine"][0] is None
    assert out["depth_filter"]["pixels"] == 6 * 48 * 64          # the integrated frames
    assert 0 < out["depth_filter"]["rejected"] < 0.05 * out["depth_filter"]["measured"]
    for rec in out["refine"][1:]:
        assert rec["fallback"] or (rec["step"][0] <= 0.1 and rec["step"][1] <= float(trunc))
    assert out["verts"].shape[0] > 1000
