"""CPU: the numpy restatement of ``ucsa_tsdf_occupancy`` (tests/occupancy_numpy.py),
which the GPU masks are held to byte for byte, and the method on the analytic room.

- The separable form (three range-ORs) equals the loop over (cell, voxel) pairs.
- Properties: a free volume that covers the box gives an all-zero mask; one
  non-free voxel keeps exactly the cells whose dilated boxes meet its box; a
  larger dilate, a larger free_tsdf and "keep" against "empty" only add cells;
  NaN keeps.
- The room of test_tsdf_fusion_cpu (room_frames(120,160), 16 views, 96^3 over
  [-3.05, 3.05]^3, trunc 4 voxels), bound 4, H 128; a surface point (a valid
  depth pixel back-projected through its pixel centre) is kept when the cell the
  marcher's lookup formula maps it to is a kept cell.  Measured with the
  restatement:

    unknown  dilate     kept c0  kept c1  kept c2  surface points in emptied cells
    keep     0          0.0162   0.2657   0.8033   0 of 307 200
    keep     one voxel  0.0477   0.3159   0.8276   0
    empty    one voxel  0        0.0030   0.1209   0
    empty    0          0        0.0017   0.0873   40

  The first three rows are asserted.  The fourth is the reason for the default
  dilate of one voxel and is not asserted: with unknown = "empty" and no
  dilation some surface points (40 by this file's back-projection) sit in
  voxels that no view observed -- beside a surface seen at a grazing angle --
  and such a voxel holds no evidence either way.
- The C marcher oracle over 1 024 rays of the room's views, mean_density 1:
  1 048 576 points with an all-ones grid (every ray runs into the 1 024-step
  cap), 188 954 with the row-3 mask as the grid (184.5 per ray): the sparsity
  figure the GPU marcher is compared with, exactly."""
import os
import re

import numpy as np
import pytest

from tests import occupancy_numpy as ON
from tests import tsdf_numpy as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

BOUND, GRID_H = 4.0, 128
ROOM_KEPT = {("keep", 0.0): (0.0162, 0.2657, 0.8033),
             ("keep", None): (0.0477, 0.3159, 0.8276),
             ("empty", None): (0.0, 0.0030, 0.1209)}
MARCH_RAYS = 1024
MARCH_POINTS_ONES = 1048576
MARCH_POINTS_PRIOR = 188954

_room = {}


def room_case():
    """The room volume (restatement), its frames and surface points; computed
    once and shared, never modified."""
    if not _room:
        from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec
        _, poses, intr, depth = room_frames(120, 160)
        dims, origin, h, trunc = room_volume_spec(96)
        vol = TN.new_volume(dims, origin, h)
        TN.integrate(vol, depth, poses, intr, trunc)
        fx, fy, cx, cy = intr
        ys, xs = np.mgrid[0:120, 0:160].astype(F32)
        ray = np.stack([(xs + 0.5 - cx) / fx, (ys + 0.5 - cy) / fy, np.ones_like(xs)],
                       -1).astype(F32)
        pts = np.concatenate([(ray * depth[b][..., None]).reshape(-1, 3) @ poses[b][:3, :3].T +
                              poses[b][:3, 3] for b in range(poses.shape[0])]).astype(F32)
        _room.update(vol=vol, poses=poses, intr=intr, depth=depth, trunc=trunc, ray=ray,
                     points=pts, masks={})
    return _room


def room_mask(unknown, dilate):
    c = room_case()
    key = (unknown, dilate)
    if key not in c["masks"]:
        v = c["vol"]
        m = ON.occupancy(v["tsdf"], v["weight"], v["origin"], v["spacing"], BOUND, None, GRID_H,
                         dilate, unknown=unknown)
        m.setflags(write=False)
        c["masks"][key] = m
    return c["masks"][key]


def room_march_rays():
    """1 024 rays through pixel centres of the room's views -> o, d, near, far"""
    from tests.util import slab_near_far
    c = room_case()
    g = np.random.default_rng(0)
    sel = g.choice(16 * 120 * 160, MARCH_RAYS, replace=False)
    b, pix = sel // (120 * 160), sel % (120 * 160)
    d = c["ray"].reshape(-1, 3)[pix]
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    dw = np.einsum("nc,nrc->nr", d, c["poses"][b][:, :3, :3]).astype(F32)
    o = np.ascontiguousarray(c["poses"][b][:, :3, 3], F32)
    near, far = slab_near_far(o, dw, BOUND)
    return o, dw, near, far


def random_volume(seed, dims):
    g = np.random.default_rng(seed)
    tsdf = np.where(g.random(dims) < 0.9, 1.0, g.uniform(-1, 1, dims)).astype(F32)
    weight = np.where(g.random(dims) < 0.9, g.integers(1, 5, dims), 0).astype(F32)
    tsdf[g.random(dims) < 0.02] = np.nan
    weight[g.random(dims) < 0.02] = np.nan
    return tsdf, weight


@pytest.mark.parametrize("seed,dims,origin,spacing,bound,cascade,H,dilate,unknown,free_tsdf", [
    (0, (7, 6, 8), (-1.2, -1.1, -1.3), (0.4, 0.45, 0.37), 2.0, 2, 4, 0.0, "keep", 1.0),
    (1, (3, 7, 2), (-2.5, -1.0, 0.2), (0.9, 0.5, 1.3), 3.0, 3, 4, 0.3, "empty", 1.0),
    (2, (6, 2, 5), (-0.5, -0.5, -0.5), (0.25, 0.5, 0.25), 1.0, 1, 5, 0.1, "empty", 0.5),
    (3, (1, 1, 1), (0.1, 0.2, -0.3), (0.5, 0.5, 0.5), 2.0, 2, 3, 0.0, "empty", 2.0),
])
def test_separable_form_is_the_definition(seed, dims, origin, spacing, bound, cascade, H, dilate,
                                          unknown, free_tsdf):
    tsdf, weight = random_volume(seed, dims)
    want = ON.occupancy_brute(tsdf, weight, origin, spacing, bound, cascade, H, dilate,
                              free_tsdf=free_tsdf, unknown=unknown)
    got = ON.occupancy(tsdf, weight, origin, spacing, bound, cascade, H, dilate,
                       free_tsdf=free_tsdf, unknown=unknown)
    assert got.dtype == np.uint8 and got.shape == (cascade, H, H, H)
    assert 0 < want.mean() < 1, want.mean()
    assert np.array_equal(got, want)


def test_free_volume_that_covers_the_box_gives_an_empty_mask():
    n = 21
    tsdf, weight = np.ones((n, n, n), F32), np.ones((n, n, n), F32)
    for unknown in ("keep", "empty"):
        m = ON.occupancy(tsdf, weight, (-2.5,) * 3, 0.25, 2.0, 2, 8, 0.25, unknown=unknown)
        assert m.shape == (2, 8, 8, 8) and not m.any()
    # the same volume unobserved: everything stays under "keep", nothing under "empty"
    assert ON.occupancy(tsdf, 0 * weight, (-2.5,) * 3, 0.25, 2.0, 2, 8, 0.25).all()
    assert not ON.occupancy(tsdf, 0 * weight, (-2.5,) * 3, 0.25, 2.0, 2, 8, 0.25,
                            unknown="empty").any()
    # a volume that ends inside the box: the cells beyond it stay under "keep"
    m = ON.occupancy(tsdf, weight, (-2.5, -2.5, -2.5), (0.25, 0.25, 0.125), 2.0, 2, 8, 0.0)
    assert not m[:, :, :, :4].any() and m[1, :, :, 5:].all()


def test_one_blocked_voxel_keeps_exactly_the_cells_that_meet_its_box():
    n, h, o = 33, 0.125, -2.0
    tsdf, weight = np.ones((n, n, n), F32), np.ones((n, n, n), F32)
    vox = (9, 20, 13)
    tsdf[vox] = 0.3
    for dilate in (0.0, 0.2):
        m = ON.occupancy(tsdf, weight, (o,) * 3, h, 2.0, 2, 8, dilate, unknown="empty")
        for cas, b in ((0, 1.0), (1, 2.0)):
            want = np.ones((8, 8, 8), bool)
            for a in range(3):
                p = o + vox[a] * h      # exact: powers of two throughout
                j = np.arange(8)
                lo, hi = b * (2 * j / 8 - 1) - dilate, b * ((2 * j + 2) / 8 - 1) + dilate
                meet = (p + h / 2 >= lo) & (p - h / 2 <= hi)
                shape = [1, 1, 1]
                shape[a] = 8
                want = want & meet.reshape(shape)
            assert want.any() or b == 1.0
            assert np.array_equal(m[cas] != 0, want), (dilate, cas)


def test_dilate_free_tsdf_and_keep_only_add_cells():
    tsdf, weight = random_volume(7, (12, 9, 14))
    tsdf = np.where(np.random.default_rng(8).random(tsdf.shape) < 0.2, F32(0.7), tsdf)
    args = ((-1.4, -1.0, -1.6), (0.25, 0.22, 0.24), 2.0, 2, 8)
    base = ON.occupancy(tsdf, weight, *args, 0.0, free_tsdf=0.5, unknown="empty")
    for more in (ON.occupancy(tsdf, weight, *args, 0.3, free_tsdf=0.5, unknown="empty"),
                 ON.occupancy(tsdf, weight, *args, 0.0, free_tsdf=1.0, unknown="empty"),
                 ON.occupancy(tsdf, weight, *args, 0.0, free_tsdf=0.5, unknown="keep")):
        assert (more >= base).all() and more.sum() > base.sum()


def test_nan_keeps():
    n = 17
    for which in ("tsdf", "weight"):
        tsdf, weight = np.ones((n, n, n), F32), np.ones((n, n, n), F32)
        (tsdf if which == "tsdf" else weight)[8, 8, 8] = np.nan
        m = ON.occupancy(tsdf, weight, (-2.0,) * 3, 0.25, 2.0, 2, 8, 0.0)
        assert m.any() and m[0, 4, 4, 4] and m[1, 4, 4, 4], which
        assert ON.not_free(tsdf, weight).sum() == 1
    # a NaN weight is "not observed": free under "empty", as everywhere else
    assert not ON.not_free(tsdf, weight, unknown="empty").any()


def test_entries_are_declared_and_bound():
    import inspect
    from ucsa_neural_rendering_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ucsa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("ucsa_tsdf_occupancy", 19), ("ucsa_tsdf_occupancy_workspace_bytes", 3)):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    sig = inspect.signature(ops.tsdf_occupancy).parameters
    assert list(sig) == ["volume", "bound", "cascade", "H", "dilate", "min_weight", "free_tsdf",
                         "unknown"]
    assert sig["H"].default == 128 and sig["unknown"].default == "keep"
    assert sig["dilate"].default is None and sig["cascade"].default is None
    mk = open(os.path.join(ROOT, "ucsa_neural_rendering_amd", "csrc", "Makefile")).read()
    line = [l for l in mk.splitlines() if "-fhip-fp32-correctly-rounded-divide-sqrt" in l][0]
    assert "occupancy_prior.o" in line and "occupancy_prior.hip" in mk


def test_renderer_prior_on_the_cpu_module():
    """set / reset / clear on a module that never saw a GPU (the Lightning hook
    applies the prior before the model moves to the device)."""
    import torch
    from ucsa_neural_rendering_amd.nerf.renderer_semantics import SemanticNeRFRenderer
    r = SemanticNeRFRenderer(bound=2, cuda_ray=True)
    keys = list(r.state_dict().keys())
    g = torch.Generator().manual_seed(0)
    mask = (torch.rand(r.density_grid.shape, generator=g) < 0.3).to(torch.uint8)
    r.density_grid.fill_(0.5)
    r.set_occupancy_prior(mask)
    assert list(r.state_dict().keys()) == keys
    assert (r.density_grid[mask == 0] == -1).all() and (r.density_grid[mask == 1] == 0.5).all()
    r.set_occupancy_prior(1 - mask)     # a new prior: the old carved cells are learnable again
    assert (r.density_grid[mask == 1] == -1).all() and (r.density_grid[mask == 0] == 0).all()
    r.reset_extra_state()
    assert (r.density_grid[mask == 1] == -1).all() and (r.density_grid[mask == 0] == 0).all()
    r.clear_occupancy_prior()
    assert (r.density_grid == 0).all() and list(r.state_dict().keys()) == keys
    r.reset_extra_state()
    assert (r.density_grid == 0).all()
    with pytest.raises(ValueError):
        r.set_occupancy_prior(mask[:1])
    with pytest.raises(ValueError):
        SemanticNeRFRenderer(bound=2).set_occupancy_prior(mask)


def test_prior_file_round_trip(tmp_path):
    from ucsa_neural_rendering_amd.utils.occupancy_prior import load_prior, save_prior
    m = (np.random.default_rng(0).random((2, 5, 5, 5)) < 0.4).astype(np.uint8)
    path = str(tmp_path / "p.npz")
    save_prior(path, m, 2.0, voxel=np.float32(0.05), unknown="empty", dilate=None)
    got, params = load_prior(path)
    assert got.dtype == np.uint8 and np.array_equal(got, m)
    assert float(params["bound"]) == 2.0 and str(params["unknown"]) == "empty"
    assert "dilate" not in params


@pytest.mark.parametrize("unknown,dilate", list(ROOM_KEPT))
def test_room_kept_shares_and_no_surface_point_is_carved(unknown, dilate):
    c = room_case()
    m = room_mask(unknown, dilate)
    kept = [float(m[cas].mean()) for cas in range(3)]
    lost = int((~ON.points_kept(m, c["points"], BOUND)).sum())
    print(f"{unknown} dilate {dilate}: kept {[round(k, 4) for k in kept]}, "
          f"{lost} of {c['points'].shape[0]} surface points in emptied cells")
    assert m.shape == (3, GRID_H, GRID_H, GRID_H) and c["points"].shape[0] == 307200
    assert lost == 0
    for got, want in zip(kept, ROOM_KEPT[(unknown, dilate)]):
        assert abs(got - want) <= 0.002


def test_room_prior_thins_the_oracle_march():
    from oracle import raymarch as orc
    o, d, near, far = room_march_rays()
    counts = []
    for grid in (np.ones((3, GRID_H, GRID_H, GRID_H), F32), room_mask("empty", None).astype(F32)):
        out = orc.march_rays_train(o, d, BOUND, grid, 1.0, near, far, force_all_rays=True)
        counts.append(int(out[4][0]))
        if grid.min() == 0:
            assert ON.points_kept(grid, out[0][:counts[-1]], BOUND).all()
    print(f"points over {MARCH_RAYS} rays: all-ones grid {counts[0]}, prior {counts[1]}")
    assert counts[1] < counts[0]
    assert counts == [MARCH_POINTS_ONES, MARCH_POINTS_PRIOR]
