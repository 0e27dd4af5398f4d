"""GPU: ``ucsa_mesh_voxelize_count`` / ``_fill`` against the numpy restatement of
their contract (tests/voxelize_numpy.py), byte for byte, with guard bytes round
the mask, the counts and the workspace; the room at H = 128 (every surface
sample in a kept cell, every kept cell at the mesh); the renderer's prior from a
mesh and the marcher on it against the C oracle's count; the two scripts."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import occupancy_numpy as ON
from tests import test_occupancy_prior_cpu as PRIOR
from tests import test_voxelize_cpu as CPU
from tests import voxelize_numpy as VN

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 4096  # bytes before and after every buffer the entries write
PATTERN = 0xA5


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared references are read-only


# ---- 1. byte for byte ----------------------------------------------------------------
def hand_mesh(fam):
    """About 40 faces placed by the family's own cell bounds (at dilate 0): a large
    quad exactly in a cell-boundary plane, a slanted triangle across the whole
    lattice, a face inside one cell, faces partly and wholly outside, a vertex
    exactly on a cell corner, a segment, a point, a NaN corner, and random faces
    -> verts float32 [V,3], faces int32 [F,3]"""
    cas = min(1, fam.ncas - 1)
    lo, hi = zip(*[fam.bounds(a, cas) for a in range(3)])
    n = fam.dims
    ext = np.array([hi[a][-1] - lo[a][0] for a in range(3)], np.float64)
    o = np.array([lo[a][0] for a in range(3)], np.float64)
    mid = [n[a] // 2 for a in range(3)]
    cell_lo = np.array([lo[a][mid[a]] for a in range(3)], np.float64)
    cell = np.array([hi[a][mid[a]] - lo[a][mid[a]] for a in range(3)], np.float64)
    g = np.random.default_rng(sum(n) + fam.ncas)
    V, Fc = [], []

    def tri(*p):
        Fc.append([len(V), len(V) + 1, len(V) + 2])
        V.extend(p)

    px = float(hi[0][n[0] // 3])                    # a plane between two x cells, exactly
    q = [[px, o[1] + 0.1 * ext[1], o[2] + 0.15 * ext[2]], [px, o[1] + 0.9 * ext[1], o[2] + 0.15 * ext[2]],
         [px, o[1] + 0.9 * ext[1], o[2] + 0.8 * ext[2]], [px, o[1] + 0.1 * ext[1], o[2] + 0.8 * ext[2]]]
    tri(q[0], q[1], q[2])
    tri(q[0], q[2], q[3])
    tri(o + 0.01 * ext, o + ext * [0.99, 0.6, 0.99], o + ext * [0.5, 0.99, 0.02])   # slanted, whole lattice
    tri(cell_lo + cell * [0.2, 0.2, 0.3], cell_lo + cell * [0.8, 0.3, 0.4],
        cell_lo + cell * [0.4, 0.7, 0.6])                                           # inside one cell
    tri(o - 0.3 * ext, o + ext * [0.3, 0.2, 0.25], o + ext * [-0.2, 0.4, 0.1])       # partly outside
    tri(o + ext * [0.8, 0.8, 1.3], o + ext * [1.4, 0.7, 0.6], o + ext * [0.7, 1.2, 0.9])
    tri(o + 3.0 * ext, o + 3.1 * ext, o + ext * [3.0, 3.2, 3.1])                    # wholly outside
    tri(o - 100.0, o - 101.0, o - [100.0, 101.0, 100.5])
    corner = np.array([hi[a][mid[a] - 1] for a in range(3)], np.float64)            # a cell corner, exactly
    tri(corner, corner + cell * [1.5, 0.4, 0.2], corner + cell * [0.3, 1.2, 0.6])
    a, b = o + ext * [0.1, 0.7, 0.3], o + ext * [0.6, 0.2, 0.75]
    tri(a, b, b)                                                                    # a segment
    tri(o + ext * [0.77, 0.31, 0.52], o + ext * [0.77, 0.31, 0.52], o + ext * [0.77, 0.31, 0.52])
    tri(o + ext * [0.3, 0.3, 0.3], [np.nan, 0.0, 0.0], o + ext * [0.5, 0.3, 0.3])    # a NaN corner
    while len(Fc) < 40:
        c = o + ext * g.uniform(0.0, 1.0, 3)
        s = ext * g.choice([0.03, 0.15, 0.4])
        tri(*(c + s * g.uniform(-1, 1, (3, 3))))
    return np.asarray(V, F32), np.asarray(Fc, np.int32)


def voxelize_guarded(V, Fc, fam, accumulate=False, start=None):
    """The two C entries with torch's prefix sum between them; the mask, the
    counts and the workspace sit inside buffers filled with a guard pattern,
    exact capacities -> mask uint8 numpy of shape ``fam.shape``"""
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    lattice = isinstance(fam, VN.Lattice)
    nv, nf = V.shape[0], Fc.shape[0]
    items = nf * fam.ncas
    cells = int(np.prod(fam.shape))
    ws_bytes = int(l.ucsa_mesh_voxelize_workspace_bytes(nf, fam.ncas))
    assert ws_bytes == 24 * items
    mbuf = torch.full((2 * GUARD + cells,), PATTERN, dtype=torch.uint8, device="cuda")
    wbuf = torch.full((2 * GUARD + ws_bytes,), PATTERN, dtype=torch.uint8, device="cuda")
    cbuf = torch.full((2 * GUARD + 4 * items,), PATTERN, dtype=torch.uint8, device="cuda")
    if start is not None:
        mbuf[GUARD:GUARD + cells] = _cu(start).reshape(-1)
    v, f = _cu(V), _cu(Fc)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    geo = (p(v), nv, p(f), nf, 0 if lattice else 1, *fam.dims,
           _lib.fvec(fam.origin.tolist()) if lattice else None,
           _lib.fvec(fam.spacing.tolist()) if lattice else None,
           0.0 if lattice else float(fam.bound), fam.ncas, float(fam.dilate))
    assert l.ucsa_mesh_voxelize_count(*geo, p(cbuf, GUARD), p(wbuf, GUARD), ws_bytes, None) == 0
    count = cbuf[GUARD:GUARD + 4 * items].view(torch.int32)
    first = torch.zeros(items + 1, dtype=torch.int64, device="cuda")
    first[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    total = int(first[items])
    assert total <= items * fam.dims[0] * fam.dims[1] and (items == 0 or int(count.min()) >= 0)
    assert l.ucsa_mesh_voxelize_fill(*geo, p(first), total, 1 if accumulate else 0, p(mbuf, GUARD),
                                     cells, p(wbuf, GUARD), ws_bytes, None) == 0
    torch.cuda.synchronize()
    for b in (mbuf, wbuf, cbuf):
        assert (b[:GUARD] == PATTERN).all() and (b[-GUARD:] == PATTERN).all()
    return mbuf[GUARD:GUARD + cells].view(fam.shape).cpu().numpy()


def _families(kind):
    """-> [(family at dilate 0, family dilated by 1.5 z-spacings)]"""
    if kind in ("blob", "slab"):
        from tests.test_gpu_occupancy_prior import contract_volume
        tsdf, _, origin, spacing = contract_volume(kind, 8)
        assert tsdf.shape == ((37, 20, 65) if kind == "blob" else (5, 3, 130))
        return [tuple(VN.Lattice(tsdf.shape, origin, spacing, d)
                      for d in (0.0, 1.5 * float(spacing[2])))]
    H = int(kind)
    return [tuple(VN.Cascade(3.0, cascade, H, d) for d in (0.0, 1.5 * 2.0 / H))
            for cascade in (1, 2, 3)]


@pytest.mark.parametrize("kind", ["8", "16", "blob", "slab"])
def test_masks_equal_the_restatement_byte_for_byte(kind):
    shares = []
    for pair in _families(kind):
        V, Fc = hand_mesh(pair[0])
        nf = len(Fc)
        assert 38 <= nf <= 44
        # through the C entries the kernels also meet indices outside [0, V)
        bad = np.array([[0, 1, V.shape[0]], [-1, 2, 3], [2 ** 31 - 1, 0, 1]], np.int32)
        Fb = np.concatenate([Fc[:7], bad, Fc[7:]])
        for fam in pair:
            want = VN.voxelize(V, Fc, fam)
            where = (kind, fam.ncas, float(fam.dilate))
            got = voxelize_guarded(V, Fb, fam)
            assert got.tobytes() == want.tobytes(), where
            assert voxelize_guarded(V, Fb, fam).tobytes() == want.tobytes(), where
            perm = np.random.default_rng(5).permutation(len(Fb))
            assert voxelize_guarded(V, Fb[perm], fam).tobytes() == want.tobytes(), where
            # two halves with accumulate, on bytes that are neither 0 nor 1 where nothing is met
            start = np.full(fam.shape, 7, np.uint8)
            half = voxelize_guarded(V, Fb[:19], fam, accumulate=True, start=start)
            both = voxelize_guarded(V, Fb[19:], fam, accumulate=True, start=half)
            assert np.array_equal(both == 1, want == 1) and np.array_equal(both == 7, want == 0), where
            shares.append(float(want.mean()))
            # no face at all: the mask is cleared, or left alone
            none = np.zeros((0, 3), np.int32)
            assert not voxelize_guarded(V, none, fam, start=start).any()
            assert (voxelize_guarded(V, none, fam, accumulate=True, start=start) == 7).all()
        # ops: the same bytes
        ops = _ops()
        fam = pair[1]
        v, f = _cu(V), _cu(Fc)
        if isinstance(fam, VN.Lattice):
            m = ops.voxelize_mesh(v, f, fam.dims, fam.origin.tolist(), fam.spacing.tolist())
            assert m.dtype == torch.uint8 and tuple(m.shape) == fam.dims and m.is_cuda
            assert m.cpu().numpy().tobytes() == VN.voxelize(V, Fc, pair[0]).tobytes()   # dilate 0
            m = ops.voxelize_mesh(v, f[:19], fam.dims, fam.origin.tolist(), fam.spacing.tolist(),
                                  dilate=float(fam.dilate))
            out = ops.voxelize_mesh(v, f[19:], fam.dims, fam.origin.tolist(),
                                    fam.spacing.tolist(), dilate=float(fam.dilate), out=m)
            assert out is m
        else:
            m = ops.mesh_occupancy(v, f, 3.0, H=fam.H)           # the renderer's cascade, one cell
            dflt = VN.Cascade(3.0, None, fam.H, None)
            assert dflt.ncas == 3 and float(dflt.dilate) == 2.0 / fam.H
            assert m.dtype == torch.uint8 and tuple(m.shape) == dflt.shape and m.is_cuda
            assert m.cpu().numpy().tobytes() == VN.voxelize(V, Fc, dflt).tobytes()
            m = ops.mesh_occupancy(v, f[:19], 3.0, cascade=fam.ncas, H=fam.H,
                                   dilate=float(fam.dilate))
            out = ops.mesh_occupancy(v, f[19:], 3.0, cascade=fam.ncas, H=fam.H,
                                     dilate=float(fam.dilate), out=m)
            assert out is m
        assert m.cpu().numpy().tobytes() == VN.voxelize(V, Fc, fam).tobytes()
    # the cases are not trivial: both kept and empty cells in most of them
    assert sum(0 < s < 1 for s in shares) >= len(shares) * 3 // 4, shares


def test_errors_from_ops_and_empty_meshes():
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    v = torch.rand(8, 3, device="cuda") - 0.5
    f = torch.tensor([[0, 1, 2], [3, 4, 5]], dtype=torch.int32, device="cuda")
    lat = ((4, 5, 6), (-0.5, -0.5, -0.5), 0.25)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(verts=v.cpu()), dict(verts=v[:, :2]), dict(verts=v.view(-1)),
                dict(faces=f.cpu()), dict(faces=f.float()), dict(faces=f[:, :2]),
                dict(faces=torch.tensor([[0, 1, 8]], dtype=torch.int32, device="cuda")),
                dict(faces=torch.tensor([[0, -1, 2]], dtype=torch.int32, device="cuda"))):
        kw = {"verts": v, "faces": f, **bad}
        with pytest.raises(UcsaError):
            ops.voxelize_mesh(kw["verts"], kw["faces"], *lat)
        with pytest.raises(UcsaError):
            ops.mesh_occupancy(kw["verts"], kw["faces"], 2.0, H=8)
    for args in (((0, 5, 6), lat[1], lat[2]), ((4, 5), lat[1], lat[2]), ((2048,) * 3, lat[1], lat[2]),
                 (lat[0], (0.0, nan, 0.0), lat[2]), (lat[0], (0.0, 0.0), lat[2]),
                 (lat[0], lat[1], 0.0), (lat[0], lat[1], (0.1, inf, 0.1)), (lat[0], lat[1], -0.1)):
        with pytest.raises(UcsaError):
            ops.voxelize_mesh(v, f, *args)
    for kw in (dict(dilate=-0.1), dict(dilate=nan), dict(dilate=inf),
               dict(out=torch.zeros(4, 5, 6, device="cuda")),
               dict(out=torch.zeros(4, 5, 7, dtype=torch.uint8, device="cuda")),
               dict(out=torch.zeros(4, 5, 6, dtype=torch.uint8))):
        with pytest.raises(UcsaError):
            ops.voxelize_mesh(v, f, *lat, **kw)
    for kw in (dict(bound=0.0), dict(bound=inf), dict(cascade=0), dict(cascade=32), dict(H=1),
               dict(H=1025), dict(dilate=-1.0), dict(dilate=nan),
               dict(out=torch.zeros(2, 8, 8, 8, device="cuda"))):
        kw = {"bound": 2.0, "H": 8, **kw}
        with pytest.raises(UcsaError):
            ops.mesh_occupancy(v, f, **kw)
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    m = ops.voxelize_mesh(v, none, *lat)
    assert tuple(m.shape) == (4, 5, 6) and not m.any()
    m = ops.mesh_occupancy(torch.zeros(0, 3, device="cuda"), none, 2.0, H=8)
    assert tuple(m.shape) == (2, 8, 8, 8) and not m.any()
    keep = torch.full((4, 5, 6), 1, dtype=torch.uint8, device="cuda")
    assert ops.voxelize_mesh(v, none, *lat, out=keep).all()          # accumulate: left alone
    assert ops.voxelize_mesh(v, f, *lat).any()


# ---- 2. the room at H = 128 ------------------------------------------------------------
@pytest.fixture(scope="module")
def room_masks():
    """step -> (V, Fc numpy, mask on the device) at bound 4, 3 cascades, dilate 0"""
    ops = _ops()
    out = {}
    for step in (1.0, 0.25):
        V, Fc = CPU.room_mesh(step)
        out[step] = (V, Fc, ops.mesh_occupancy(_cu(V), _cu(Fc), PRIOR.BOUND, dilate=0.0))
    return out


@pytest.mark.parametrize("step", [1.0, 0.25])
def test_room_surface_samples_are_kept_and_kept_cells_touch_the_mesh(room_masks, step):
    ops = _ops()
    V, Fc, mask = room_masks[step]
    assert tuple(mask.shape) == (3, 128, 128, 128)
    v, f = _cu(V), _cu(Fc)
    pts = ops.sample_mesh_surface(v, f, 900.0, seed=3)["points"].cpu().numpy()
    assert pts.shape[0] > 150000
    fam = VN.Cascade(PRIOR.BOUND, 3, 128, 0.0)
    grid = ops.triangle_grid(v, f)

    def nearest(c):
        index, dist2, _ = ops.nearest_triangle(grid, _cu(c), 1.0)
        assert (index >= 0).all()
        return dist2.double().sqrt().cpu().numpy()

    m = mask.cpu().numpy()
    worst = CPU.check_room_mask(m, fam, V, Fc, pts, nearest)
    kept = [round(float(m[c].mean()), 4) for c in range(3)]
    print(f"\nroom step {step}: {len(Fc)} faces, H 128, dilate 0: kept {kept}; {pts.shape[0]} "
          f"surface samples, all in kept cells; {int(m.sum())} kept cells, worst centre distance "
          f"- reach {worst:.3g}")
    assert 0 < kept[2] < 0.5


# ---- 3. the renderer ---------------------------------------------------------------------
def test_renderer_takes_the_mesh_prior_and_the_marcher_matches_the_oracle(room_masks):
    from oracle import raymarch as orc
    from ucsa_neural_rendering_amd.nerf.network_tcnn_semantics import SemanticNeRFNetwork
    from ucsa_neural_rendering_amd.nerf.raymarching import raymarching as rm
    mask = room_masks[0.25][2]
    carved = mask == 0
    net = SemanticNeRFNetwork(encoding="hashgrid", bound=4, cuda_ray=True,
                              num_semantic_classes=8, seed=3).cuda().eval()
    keys = list(net.state_dict().keys())
    o, d, near, far = PRIOR.room_march_rays()

    def march(grid, mean):
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        xyzs = rm.march_rays_train(_cu(o), _cu(d), PRIOR.BOUND, grid, mean, _cu(near), _cu(far),
                                   cnt, -1, False, -1, True, 0.0)[0]
        return cnt.tolist(), xyzs

    # step 0: one init of the grid from the fresh field, one ray batch
    net.update_extra_state()
    plain, _ = march(net.density_grid, net.mean_density)
    net.set_occupancy_prior(mask)
    assert list(net.state_dict().keys()) == keys
    assert torch.equal(net.occupancy_prior, mask)
    assert (net.density_grid[carved] == -1).all() and (net.density_grid[~carved] >= 0).all()
    prior, xyzs = march(net.density_grid, net.mean_density)
    assert prior[1] == plain[1] == PRIOR.MARCH_RAYS
    assert prior[0] < plain[0]          # <= in general, strictly fewer on the room
    assert ON.points_kept(mask.cpu().numpy(), xyzs.cpu().numpy(), PRIOR.BOUND).all()
    print(f"\nstep 0, {PRIOR.MARCH_RAYS} rays: {plain[0]} points without the prior, {prior[0]} with")
    net.update_extra_state()
    assert (net.density_grid[carved] == -1).all() and (net.density_grid[~carved] >= 0).all()
    net.reset_extra_state()
    assert (net.density_grid[carved] == -1).all() and (net.density_grid[~carved] == 0).all()
    net.clear_occupancy_prior()
    assert (net.density_grid == 0).all() and getattr(net, "occupancy_prior", None) is None
    assert list(net.state_dict().keys()) == keys
    # the mask as the grid, mean_density 1: the C oracle's point count, exactly
    m = mask.cpu().numpy().astype(F32)
    want = orc.march_rays_train(o, d, PRIOR.BOUND, m, 1.0, near, far, force_all_rays=True)
    got, xyzs = march(_cu(m), 1.0)
    assert got == [int(want[4][0]), PRIOR.MARCH_RAYS] and 0 < got[0] < PRIOR.MARCH_POINTS_ONES
    assert xyzs.shape[0] == got[0]


# ---- 4. the scripts ------------------------------------------------------------------------
def test_occupancy_prior_script_mesh_route_and_the_lightning_hook(tmp_path, capsys, room_masks):
    from scripts import occupancy_prior as script
    from tests.test_gpu_losses_and_module import _tiny_exp
    from ucsa_neural_rendering_amd.lightning import JointTrainLightningNet
    from ucsa_neural_rendering_amd.utils.occupancy_prior import load_prior
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    from ucsa_neural_rendering_amd.utils.semantic_mesh import ngp_to_pose_frame
    ops = _ops()
    V, Fc, _ = room_masks[0.25]
    write_ply(str(tmp_path / "room.ply"), V, Fc)
    out = str(tmp_path / "prior" / "prior.npz")
    rec = script.main(["--mesh", str(tmp_path / "room.ply"), "--out", out])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("occupancy_prior: ")]
    assert len(lines) == 1
    line = json.loads(lines[0][len("occupancy_prior: "):])
    assert line == json.loads(json.dumps(rec))
    assert line["source"] == "mesh" and line["faces"] == len(Fc) and line["skipped"] == 0
    assert line["cascade"] == 3 and line["H"] == 128 and len(line["kept"]) == 3
    assert 0 < line["kept"][2] < 0.5 and line["voxelize_ms"] > 0
    assert os.path.getsize(out) < 1 << 20
    mask, params = load_prior(out)
    want = ops.mesh_occupancy(_cu(V), _cu(Fc), 4.0)               # the op's defaults
    assert mask.dtype == np.uint8 and np.array_equal(mask, want.cpu().numpy())
    assert str(params["source"]) == "mesh" and float(params["bound"]) == 4.0
    assert float(params["dilate"]) == float(F32(2.0 / 128))
    # the same mesh in the pose frame, other bound / dilate / H
    write_ply(str(tmp_path / "pose.ply"), ngp_to_pose_frame(V).astype(F32), Fc)
    out2 = str(tmp_path / "pose.npz")
    script.main(["--mesh", str(tmp_path / "pose.ply"), "--mesh_pose_frame", "--out", out2,
                 "--bound", "3.5", "--dilate", "0", "--H", "32"])
    mask2, _ = load_prior(out2)
    want2 = ops.mesh_occupancy(_cu(V), _cu(Fc), 3.5, H=32, dilate=0.0)
    assert mask2.shape == (3, 32, 32, 32) and np.array_equal(mask2, want2.cpu().numpy())
    with pytest.raises(SystemExit):
        script.main(["--out", out])                              # neither route
    with pytest.raises(SystemExit):
        script.main(["--mesh", "m.ply", "--scene_root", "s", "--out", out])
    capsys.readouterr()
    # the experiment key
    env = {"results": str(tmp_path), "scannet": str(tmp_path)}
    exp = _tiny_exp()
    exp["nerf"].update(cuda_ray=True, occupancy_prior=out)
    model = JointTrainLightningNet(exp, env).cuda()
    grid = model.nerf_model.density_grid
    assert torch.equal(model.nerf_model.occupancy_prior.cpu(), torch.from_numpy(mask))
    assert torch.equal(grid < 0, _cu(mask) == 0) and (grid[grid >= 0] == 0).all()


def test_score_mesh_3d_voxel_iou(tmp_path, capsys):
    from scripts import score_mesh_3d
    from tests.test_gpu_sample import HOLE_FACE, HOLE_R
    from tests.test_surface_cpu import room
    from ucsa_neural_rendering_amd.utils.mesh_eval import voxel_iou
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    ops = _ops()
    m = room()
    gt, fine = m["coarse"], m["fine"]
    fv, ff = fine["verts"].astype(F32), fine["faces"].astype(np.int32)
    t = gt["verts"][gt["faces"][HOLE_FACE]].astype(np.float64)
    side = [np.linalg.norm(t[1] - t[2]), np.linalg.norm(t[0] - t[2]), np.linalg.norm(t[0] - t[1])]
    centre = (side[0] * t[0] + side[1] * t[1] + side[2] * t[2]) / sum(side)
    gone = (np.linalg.norm(fv.astype(np.float64) - centre, axis=1)[ff] <= HOLE_R).all(1)
    assert 0 < gone.sum() < len(ff)
    write_ply(str(tmp_path / "whole.ply"), fv, ff)
    write_ply(str(tmp_path / "holed.ply"), fv, ff[~gone])
    base = ["--gt", str(tmp_path / "whole.ply"), "--max_dist", "0.2", "--threshold", "0.01"]

    def geometry(pred, *flags):
        rec = score_mesh_3d.main(["--pred", str(tmp_path / pred)] + base + list(flags))
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("geometry: ")]
        assert len(lines) == 1 and json.loads(lines[0][len("geometry: "):]) == \
            json.loads(json.dumps(rec["geometry"]))
        return rec["geometry"]

    VOXEL = 0.1
    plain = geometry("whole.ply")
    assert "voxel_iou" not in plain                       # without the flag: as before
    same = geometry("whole.ply", "--voxel_iou", str(VOXEL))
    assert {k: v for k, v in same.items() if k != "voxel_iou"} == plain
    s = same["voxel_iou"]
    assert s["iou"] == 1.0 and s["precision"] == 1.0 and s["recall"] == 1.0
    assert s["n_pred"] == s["n_gt"] > 1000 and s["voxel"] == float(F32(VOXEL))
    h = geometry("holed.ply", "--voxel_iou", str(VOXEL))["voxel_iou"]
    assert h["precision"] == 1.0 and h["n_gt"] == s["n_gt"]
    assert h["recall"] < 1.0 and h["iou"] == h["recall"] and h["n_pred"] < h["n_gt"]
    # the missing voxels meet only removed faces, which lie in the ball of radius HOLE_R
    # round the disc's centre: their centres are within HOLE_R + half a diagonal of it
    dims, origin = VN.iou_lattice(fv, fv, VOXEL)
    assert list(dims) == h["dims"]
    args = (dims, origin.tolist(), float(F32(VOXEL)))
    G = ops.voxelize_mesh(_cu(fv), _cu(ff), *args) != 0
    P = ops.voxelize_mesh(_cu(fv), _cu(ff[~gone]), *args) != 0
    assert int(G.sum()) == h["n_gt"] and int(P.sum()) == h["n_pred"] and not (P & ~G).any()
    idx = torch.nonzero(G & ~P).cpu().numpy()
    assert len(idx) == h["n_gt"] - h["n_pred"] > 0
    c = origin.astype(np.float64) + idx * float(F32(VOXEL))
    assert (np.linalg.norm(c - centre, axis=1) <= HOLE_R + 0.5 * np.sqrt(3.0) * VOXEL + 1e-6).all()
    print(f"\nvoxel IoU at {VOXEL}: {s['n_gt']} voxels; the holed mesh misses {len(idx)}: "
          f"recall {h['recall']:.4f}")
    with pytest.raises(ValueError):
        voxel_iou(fv, ff, fv, ff, 1e-4)                   # 60 000^3 voxels: refused before allocating
    assert voxel_iou(fv, ff, fv, ff, 0.5, dilate=0.1, max_voxels=20 ** 3)["iou"] == 1.0
