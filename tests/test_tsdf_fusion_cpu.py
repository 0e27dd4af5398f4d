"""CPU: the numpy restatement of the TSDF contracts (tests/tsdf_numpy.py), which
the GPU volumes and meshes are held to bit for bit, and the method itself on the
analytic room.

- Properties of the integration: a fronto-parallel plane gives the exact ramp;
  any split of the views over calls gives the same bytes; invalid depths,
  pixels outside the image and voxels behind the camera change nothing;
  max_weight clamps; colour averages.
- Masked marching cubes: an all-ones mask is ``mc_numpy.marching_cubes``; no
  vertex on an edge with an invalid end; a half-masked sphere is the unmasked
  run of the valid half.
- The C entries are declared in the header and in the ctypes table.
- The room: depth frames -> volume -> mesh lies on the room; the mask removes the
  sheet behind the boxes that unmasked marching cubes of -tsdf shows."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mc_numpy as M
from tests import tsdf_numpy as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [4,4] f32, +z forward, columns (right, down, forward)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = r, np.cross(f, r), f, eye
    return P.astype(F32)


RANDOM_DIMS, RANDOM_H, RANDOM_W = (37, 20, 65), 48, 64
RANDOM_INTR = (60.0, 57.0, 31.3, 24.6)


def random_case(seed=0, views=16):
    """Odd dims (partial waves and bricks), cameras around the volume, two of
    them looking away from it and two inside it, depth maps with every kind of
    invalid value sprinkled in, random colours.  -> dict"""
    g = np.random.default_rng(seed)
    origin = np.array([-0.9, 0.4, -1.7], F32)
    spacing = np.array([0.05, 0.06, 0.055], F32)
    ext = (np.array(RANDOM_DIMS) - 1) * spacing.astype(np.float64)
    centre = origin + ext / 2
    poses, depth = [], []
    for b in range(views):
        d = g.normal(size=3)
        d /= np.linalg.norm(d)
        eye = centre + d * g.uniform(2.5, 4.0)
        target = centre + g.uniform(-0.3, 0.3, 3) * ext
        if b in (3, 11):
            target = eye + (eye - centre)          # looks away from the volume
        if b in (5, 13):
            eye = centre + g.uniform(-0.2, 0.2, 3) * ext   # inside the volume
        poses.append(look_at(eye, target, up=g.normal(size=3)))
        dist = np.linalg.norm(eye - centre)
        ys, xs = np.mgrid[0:RANDOM_H, 0:RANDOM_W]
        z = dist + 0.6 * np.sin(xs / 9.0 + b) * np.cos(ys / 7.0 - b) + g.normal(0, 0.02, xs.shape)
        if b in (5, 13):
            z = 0.5 + 0.3 * np.sin(xs / 5.0) + 0.0 * ys
        z = z.astype(F32)
        z[g.random(z.shape) < 0.03] = 0.0
        z[g.random(z.shape) < 0.02] = np.nan
        z[g.random(z.shape) < 0.01] = np.inf
        z[g.random(z.shape) < 0.01] = -np.inf
        z[g.random(z.shape) < 0.02] *= -1.0
        z[g.random(z.shape) < 0.02] = 9.0          # beyond depth_max
        depth.append(z)
    color = g.integers(0, 256, (views, RANDOM_H, RANDOM_W, 3)).astype(np.uint8)
    return {"dims": RANDOM_DIMS, "origin": origin, "spacing": spacing, "poses": np.stack(poses),
            "depth": np.stack(depth), "color": color, "intr": RANDOM_INTR, "trunc": 0.22,
            "max_weight": 11.0, "depth_min": 0.05, "depth_max": 8.0}


def run_numpy(case, splits, with_color=True):
    """the case integrated in calls of the views [a, b) of ``splits``"""
    vol = TN.new_volume(case["dims"], case["origin"], case["spacing"], with_color)
    for a, b in splits:
        TN.integrate(vol, case["depth"][a:b], case["poses"][a:b], case["intr"], case["trunc"],
                     color=case["color"][a:b] if with_color else None,
                     max_weight=case["max_weight"], depth_min=case["depth_min"],
                     depth_max=case["depth_max"])
    return vol


def batches(n, size):
    return [(a, min(a + size, n)) for a in range(0, n, size)]


def same_bytes(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes()
               for k in ("tsdf", "weight", "rgb"))


def test_fronto_parallel_plane_gives_the_exact_ramp():
    # powers of two throughout: every product, quotient and sum below is exact
    n, h, z0, trunc = 33, F32(0.125), F32(2.0), F32(0.5)
    vol = TN.new_volume((n, n, n), (-2.0, -2.0, 0.125), h)
    H = W = 64
    intr = (64.0, 64.0, 32.0, 32.0)
    depth = np.full((1, H, W), z0, F32)
    TN.integrate(vol, depth, np.eye(4, dtype=F32)[None], intr, trunc)
    x, y, z = (a.astype(np.float64) for a in TN.voxel_centres(vol))
    u, v = np.floor(64.0 * x / z + 32.0), np.floor(64.0 * y / z + 32.0)
    seen = np.broadcast_to((u >= 0) & (u < W) & (v >= 0) & (v < H), vol["tsdf"].shape)
    zz = np.broadcast_to(z, vol["tsdf"].shape)
    front = seen & (zz < z0 - trunc)
    band = seen & (zz >= z0 - trunc) & (zz <= z0 + trunc)
    behind = zz > z0 + trunc
    assert front.sum() > 100 and band.sum() > 1000 and behind.sum() > 1000
    assert (vol["tsdf"][front] == 1).all() and (vol["weight"][front] == 1).all()
    assert np.array_equal(vol["tsdf"][band], ((z0 - zz[band]) / trunc).astype(F32))
    assert (vol["weight"][band] == 1).all()
    assert (vol["weight"][behind] == 0).all() and (vol["tsdf"][behind] == 1).all()
    assert (vol["weight"][~seen] == 0).all()
    assert vol["tsdf"].min() == -1.0  # the far end of the band is inside it


def test_any_split_of_the_views_gives_the_same_bytes():
    case = random_case(0, views=7)
    one = run_numpy(case, [(0, 7)])
    assert 0.2 < (one["weight"] > 0).mean() < 1.0
    assert one["weight"].max() > 3 and one["tsdf"].min() < -0.5
    assert same_bytes(one, run_numpy(case, batches(7, 1)))
    assert same_bytes(one, run_numpy(case, [(0, 2), (2, 2), (2, 3), (3, 7)]))
    no_color = run_numpy(case, [(0, 7)], with_color=False)
    assert no_color["rgb"] is None
    assert no_color["tsdf"].tobytes() == one["tsdf"].tobytes()
    # the order of views matters to the bits (a running average), which is why
    # the contract fixes it
    assert (one["rgb"][one["weight"] > 0] > 0).any()


def test_invalid_depths_outside_pixels_and_voxels_behind_change_nothing():
    case = random_case(1, views=1)
    base = TN.new_volume(case["dims"], case["origin"], case["spacing"], True)
    centre = case["origin"] + (np.array(case["dims"]) - 1) * case["spacing"] / 2
    eye = centre + np.array([3.0, 0.5, 0.2])
    toward, away = look_at(eye, centre), look_at(eye, 2 * eye - centre)
    aside = look_at(eye, eye + np.array([0.0, 1.0, 0.0]))  # in front, outside the image
    good = np.full((1, RANDOM_H, RANDOM_W), 3.0, F32)
    col = np.full((1, RANDOM_H, RANDOM_W, 3), 200, np.uint8)
    kw = dict(color=col, depth_min=0.05, depth_max=8.0)
    for bad in (0.0, np.nan, np.inf, -np.inf, -3.0, 0.04, 8.5):
        vol = TN.integrate({k: (v.copy() if v is not None else v) for k, v in base.items()},
                           np.full_like(good, bad), toward[None], RANDOM_INTR, 0.22, **kw)
        assert same_bytes(vol, base), bad
    for pose in (away, aside):
        vol = TN.integrate({k: (v.copy() if v is not None else v) for k, v in base.items()},
                           good, pose[None], RANDOM_INTR, 0.22, **kw)
        assert same_bytes(vol, base)
    vol = TN.integrate({k: (v.copy() if v is not None else v) for k, v in base.items()},
                       good, toward[None], RANDOM_INTR, 0.22, **kw)
    assert (vol["weight"] == 1).sum() > 1000  # the same set-up with a valid view does


def test_max_weight_clamps_and_colour_averages():
    case = random_case(2, views=1)
    vol = TN.new_volume(case["dims"], case["origin"], case["spacing"], True)
    depth = np.nan_to_num(np.abs(case["depth"]), nan=3.0, posinf=3.0)
    depth[depth > 8] = 3.0
    depth[depth < 0.05] = 3.0
    for value in (10, 20, 60, 60, 60):
        TN.integrate(vol, depth, case["poses"], case["intr"], 0.22,
                     color=np.full_like(case["color"], value), max_weight=3.0)
    w = vol["weight"]
    seen = w > 0
    assert seen.sum() > 1000 and (w[seen] == 3).all()  # one view: every voxel seen 5 times
    # (10 + 20)/2 = 15, (15*2 + 60)/3 = 30, then weight stays 3: (30*3 + 60)/4
    want = F32(F32(30 * 3 + 60) / F32(4))
    want = F32((want * F32(3) + F32(60)) / F32(4))
    assert (vol["rgb"][seen] == want).all() and (vol["rgb"][~seen] == 0).all()
    with pytest.raises(ValueError):
        TN.integrate(vol, depth, case["poses"], case["intr"], 0.22)


def _smooth_field(seed, dims):
    g = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n) for n in dims], indexing="ij")
    f = np.sin(3 * x + g.uniform(0, 3)) * np.cos(2.5 * y + g.uniform(0, 3)) + 0.7 * np.sin(
        4 * z + g.uniform(0, 3)) * x
    return f.astype(F32)


def test_all_ones_mask_is_the_unmasked_marching_cubes():
    f = _smooth_field(0, (19, 14, 23))
    o, h = (0.3, -1.0, 2.0), (0.1, 0.07, 0.13)
    want = M.marching_cubes(f, 0.1, o, h)
    got = TN.marching_cubes_masked(f, 0.1, np.ones(f.shape, np.uint8), o, h)
    assert want[0].shape[0] > 500
    for a, b in zip(want, got):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_random_mask_leaves_no_vertex_on_an_edge_with_an_invalid_end():
    f = _smooth_field(1, (21, 17, 18))
    valid = np.random.default_rng(5).random(f.shape) < 0.9
    o, h = (0.0, 0.0, 0.0), (0.5, 0.25, 1.0)
    v, faces, n = TN.marching_cubes_masked(f, 0.0, valid, o, h)
    full = M.marching_cubes(f, 0.0, o, h)
    assert 100 < v.shape[0] < full[0].shape[0] and 0 < faces.shape[0] < full[1].shape[0]
    assert faces.min() >= 0 and faces.max() < v.shape[0]
    lo, hi = TN.vertex_edges(v, o, h, f.shape)
    assert valid[lo[:, 0], lo[:, 1], lo[:, 2]].all() and valid[hi[:, 0], hi[:, 1], hi[:, 2]].all()
    assert np.isfinite(n).all()
    # every masked vertex is a vertex of the unmasked run, bit for bit
    assert {r.tobytes() for r in v} <= {r.tobytes() for r in full[0]}


def test_half_masked_sphere_is_the_unmasked_run_of_the_valid_half():
    n, m = 24, 13
    x, y, z = np.meshgrid(*[np.linspace(-1.2, 1.2, n).astype(F32)] * 3, indexing="ij")
    f = (F32(0.8) - np.sqrt(x * x + y * y + z * z)).astype(F32)  # inside > 0
    valid = np.zeros(f.shape, bool)
    valid[:m + 1] = True
    o, h = (-1.2, -1.2, -1.2), (0.1, 0.1, 0.1)
    got = TN.marching_cubes_masked(f, 0.0, valid, o, h)
    near = M.marching_cubes(f[:m + 1], 0.0, o, h)  # the valid half as a lattice of its own
    for a, b in zip(near, got):
        assert a.tobytes() == b.tobytes()
    full_v, full_f, _ = M.marching_cubes(f, 0.0, o, h)
    F = got[1].shape[0]
    assert 0 < F < full_f.shape[0]
    # cells come in ascending index: the valid half's triangles are the first F
    assert np.array_equal(got[0][got[1]], full_v[full_f[:F]])


def test_entries_are_declared_and_bound():
    from ucsa_neural_rendering_amd import _lib
    src = open(os.path.join(ROOT, "include", "ucsa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("ucsa_tsdf_integrate", 23), ("ucsa_mc_count_masked", 9),
                        ("ucsa_mc_emit_masked", 15)):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    from ucsa_neural_rendering_amd import ops
    assert callable(ops.integrate_tsdf) and callable(ops.tsdf_volume)
    import inspect
    assert inspect.signature(ops.marching_cubes).parameters["valid"].default is None
    mk = open(os.path.join(ROOT, "ucsa_neural_rendering_amd", "csrc", "Makefile")).read()
    line = [l for l in mk.splitlines() if "-fhip-fp32-correctly-rounded-divide-sqrt" in l][0]
    assert "tsdf_fusion.o" in line and "marching_cubes.o" in line


# ---- the method on the analytic room ---------------------------------------
ROOM_LO, ROOM_HI = -3.05, 3.05
TRUNC_VOXELS = 4
# Measured with this restatement (the GPU path is bit-identical to it): 16 views of
# _slerp_loop_poses(16, seed=123), z-depth from SyntheticRoom.cast through the
# pixel centres, volume over [-3.05, 3.05]^3, trunc = 4 voxels, mask weight >= 1;
# vertex-to-room distance (SyntheticRoom.nearest_surface) in voxels:
#   96^3, 120x160:  61.1 % of the voxels observed; unmasked 30 388 vertices, 1 799
#     of them on an edge with an unobserved end (95th percentile 0.779); masked
#     28 589 vertices, none on such an edge, median 0.0280, 95th percentile
#     0.1084, maximum 2.750
#   128^3, 240x320, depth through the uint16-millimetre PNG (the end-to-end test
#     of tests/test_gpu_tsdf_fusion.py): 66 669 vertices, 0.0344 / 0.0693 / 3.424
# Bounds: the 96^3 figures plus a quarter of a voxel (median) and one voxel (95th
# percentile), the discretisation scale of the method; no vertex farther than
# trunc + one voxel (a vertex sits between an observed-inside voxel, which lies
# within trunc behind a measured surface point, and its neighbour).
MEDIAN_MAX_VOXELS = 0.0280 + 0.25
P95_MAX_VOXELS = 0.1084 + 1.0
FARTHEST_MAX_VOXELS = TRUNC_VOXELS + 1.0


def room_frames(H, W, views=16):
    """poses [views,4,4], intrinsics, z-depth [views,H,W] f32 of SyntheticRoom(0)"""
    from tests.test_mesh_raster_cpu import cast_room
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, \
        _slerp_loop_poses
    room = SyntheticRoom(0)
    poses = _slerp_loop_poses(views, seed=123).numpy()
    intr = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    depth = np.stack([cast_room(room, poses[b], intr, H, W)[0] for b in range(views)])
    return room, poses, intr, depth.astype(F32)


def room_volume_spec(n):
    h = F32((ROOM_HI - ROOM_LO) / (n - 1))
    return (n, n, n), (ROOM_LO,) * 3, h, F32(TRUNC_VOXELS * h)


def vertex_distance_voxels(room, verts, h):
    return room.nearest_surface(torch.from_numpy(np.asarray(verts, F32)))[0].numpy() / float(h)


def check_distance_bounds(d):
    """d: vertex-to-room distances in voxels"""
    assert np.median(d) <= MEDIAN_MAX_VOXELS
    assert np.percentile(d, 95) <= P95_MAX_VOXELS
    assert d.max() <= FARTHEST_MAX_VOXELS


def test_room_mesh_lies_on_the_room_and_the_mask_removes_the_back_sheet():
    room, poses, intr, depth = room_frames(120, 160)
    dims, origin, h, trunc = room_volume_spec(96)
    vol = TN.new_volume(dims, origin, h)
    TN.integrate(vol, depth, poses, intr, trunc)
    valid = vol["weight"] >= 1
    assert 0.5 < valid.mean() < 0.75
    v, f, n = TN.extract(vol)
    d = vertex_distance_voxels(room, v, h)
    print(f"observed {valid.mean():.4f}; masked: {v.shape[0]} vertices, {f.shape[0]} faces, "
          f"distance in voxels median {np.median(d):.4f}, p95 {np.percentile(d, 95):.4f}, "
          f"max {d.max():.4f}")
    assert v.shape[0] > 20000
    check_distance_bounds(d)

    def on_unobserved_edges(verts):
        lo, hi = TN.vertex_edges(verts, vol["origin"], vol["spacing"], dims)
        return int((~(valid[lo[:, 0], lo[:, 1], lo[:, 2]] &
                      valid[hi[:, 0], hi[:, 1], hi[:, 2]])).sum())

    v_all = M.marching_cubes(-vol["tsdf"], 0.0, vol["origin"], vol["spacing"])[0]
    d_all = vertex_distance_voxels(room, v_all, h)
    print(f"unmasked: {v_all.shape[0]} vertices, {on_unobserved_edges(v_all)} on edges with an "
          f"unobserved end, p95 {np.percentile(d_all, 95):.4f}")
    assert on_unobserved_edges(v_all) > 0
    assert on_unobserved_edges(v) == 0
