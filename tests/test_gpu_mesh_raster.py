"""GPU: the mesh rasterizer (csrc/mesh_raster.hip, ops.rasterize_mesh).

- tri_id, label, depth and rgb BIT-identical to the numpy restatement of the
  contract (tests/raster_numpy.py) on a seeded triangle soup, the analytic
  room at two grid steps and two sizes, an empty mesh and an off-screen mesh;
  two runs give the same bytes.
- The capacity contract through ctypes, with guard bytes after each buffer.
- Argument errors raise UcsaError.
- End to end: scripts/render_mesh_labels.py on an exported synthetic scene
  against its label_40 / depth PNGs, and --score."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from tests import raster_numpy as R
from tests.test_mesh_raster_cpu import ROOM_AGREE_MIN, room_views

pytestmark = pytest.mark.gpu


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.int32)


def _gpu(verts, faces, poses, intr, H, W, near, labels=None, rgb=None):
    cu = lambda a, dt=None: None if a is None else torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a if dt is None else np.asarray(a, dt))).cuda()
    out = _ops().rasterize_mesh(cu(verts, np.float32), cu(faces, np.int32),
                                cu(poses, np.float32), intr, H, W, near,
                                vertex_labels=cu(labels, np.int32),
                                vertex_rgb=cu(rgb, np.float32))
    torch.cuda.synchronize()
    return out


def _check_exact(verts, faces, poses, intr, H, W, near, labels=None, rgb=None):
    got = _gpu(verts, faces, poses, intr, H, W, near, labels, rgb)
    ref = R.rasterize(verts, faces, poses, intr, H, W, near, labels, rgb)
    assert got["tri_id"].dtype == torch.int32 and got["label"].dtype == torch.int32
    assert tuple(got["tri_id"].shape) == (poses.shape[0], H, W)
    for k in ("tri_id", "label"):
        assert np.array_equal(got[k].cpu().numpy(), ref[k]), k
    assert np.array_equal(_bits(got["depth"]), _bits(ref["depth"]))
    if rgb is not None:
        assert np.array_equal(_bits(got["rgb"]), _bits(ref["rgb"]))
    else:
        assert "rgb" not in got
    again = _gpu(verts, faces, poses, intr, H, W, near, labels, rgb)
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), ("second run", k)
    return got, ref


def _look_at(eye, target):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, d, f, eye
    return m.astype(np.float32)


def _soup(seed=11, n=400):
    g = np.random.default_rng(seed)
    V = []
    faces = []
    for i in range(n):
        kind = i % 8
        c = g.uniform([-2, -2, -1], [2, 2, 1])
        if kind == 0:    # degenerate: a repeated corner / collinear corners
            p = np.stack([c, c, c + g.normal(size=3) * 0.3])
            if i % 16 == 0:
                p[1] = (p[0] + p[2]) / 2
        elif kind == 1:  # huge
            p = c + g.normal(size=(3, 3)) * 1e3
        elif kind == 2:  # behind the camera (the camera sits at y = -5)
            p = np.array([0, -8, 0]) + g.normal(size=(3, 3))
        elif kind == 3:  # crossing the near plane
            p = np.array([0, -5, 0]) + g.normal(size=(3, 3)) * 1.5
        else:
            p = c + g.normal(size=(3, 3)) * 0.4
        base = len(V) * 3
        V.append(p)
        tri = [base, base + 1, base + 2]
        if g.random() < 0.5:
            tri = tri[::-1]
        faces.append(tri)
        if kind == 4:    # a coplanar overlap: the same triangle again, other winding
            faces.append([base, base + 2, base + 1])
    verts = np.concatenate(V).astype(np.float32)
    faces = np.array(faces, np.int32)
    labels = g.integers(0, 41, verts.shape[0]).astype(np.int32)
    rgb = g.random((verts.shape[0], 3)).astype(np.float32)
    poses = np.stack([_look_at([0.3, -5, 0.4], [0, 0, 0]),
                      _look_at([4, -3, 2], [0, 0, -0.5]),
                      _look_at([0, -5.5, 0], [0, -8, 0.1])])
    return verts, faces, labels, rgb, poses


def test_soup_bit_exact_against_numpy():
    verts, faces, labels, rgb, poses = _soup()
    got, ref = _check_exact(verts, faces, poses, (90.0, 95.0, 61.3, 47.9), 96, 128, 0.1,
                            labels, rgb)
    assert (ref["tri_id"] >= 0).mean() > 0.2


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
    rgb = room.palette.cpu().numpy()[m["labels"] - 1].astype(np.float32)
    poses, intr = room_views(H, W)
    got, ref = _check_exact(m["verts"], m["faces"], poses, intr, H, W, 0.05, m["labels"], rgb)
    assert (ref["tri_id"] >= 0).mean() > 0.99


def test_empty_and_offscreen_meshes():
    poses = np.stack([np.eye(4, dtype=np.float32)] * 2)
    intr = (64.0, 64.0, 32.0, 24.0)
    got, _ = _check_exact(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), poses,
                          intr, 48, 64, 0.1)
    assert (got["tri_id"] == -1).all() and (got["depth"] == 0).all()
    assert (got["label"] == 0).all()
    # a mesh wholly beside the view, and one behind the camera
    verts = np.array([[50, 0, 1], [51, 0, 1], [50, 1, 1], [0, 0, -2], [1, 0, -2], [0, 1, -2]],
                     np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    got, _ = _check_exact(verts, faces, poses, intr, 48, 64, 0.1,
                          np.array([3] * 6, np.int32), np.ones((6, 3), np.float32))
    assert (got["tri_id"] == -1).all() and (got["rgb"] == 0).all()


def test_capacity_contract_through_ctypes():
    from ucsa_neural_rendering_amd import _lib
    lib = _lib.lib()
    verts, faces, labels, rgb, poses = _soup(seed=3, n=120)
    H, W, B = 40, 56, poses.shape[0]
    V, F = verts.shape[0], faces.shape[0]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tv, tf, tp, tl, tr = cu(verts), cu(faces), cu(poses), cu(labels), cu(rgb)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    intr = (60.0, 60.0, 28.0, 20.0)
    args = (p(tv), V, p(tf), F, p(tp), B, *intr, H, W, 0.1)
    ws = torch.empty(int(lib.ucsa_raster_workspace_bytes(B, F, H, W)), dtype=torch.uint8,
                     device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ucsa_raster_setup(*args, p(ws), p(total), stream) == 0
    n = int(total.item())
    assert n > 0
    GUARD = 64
    N = B * H * W

    def bufs(n_pairs, n_pix):
        fill = lambda k, dt: torch.full((k + GUARD,), 0x5A5A5A5A, dtype=dt,  # noqa: E731
                                        device="cuda") if dt == torch.int32 else \
            torch.full((k + GUARD,), 1234.5, dtype=dt, device="cuda")
        return (fill(n_pairs, torch.int32), fill(n_pix, torch.int32), fill(n_pix, torch.float32),
                fill(n_pix, torch.int32), fill(3 * n_pix, torch.float32))

    def draw(b, total_pairs, max_pairs, max_pix):
        return lib.ucsa_raster_draw(*args, p(tl), p(tr), p(ws), p(b[0]), total_pairs, max_pairs,
                                    p(b[1]), p(b[2]), p(b[3]), p(b[4]), max_pix, stream)

    # too few pair slots, too few pixels: an argument error, nothing written
    for n_pairs, n_pix, code in ((n - 1, N, -1018), (n, N - 1, -1023)):
        b = bufs(n_pairs, n_pix)
        snap = [x.clone() for x in b]
        assert draw(b, n, n_pairs, n_pix) == code
        torch.cuda.synchronize()
        for x, y in zip(b, snap):
            assert torch.equal(x, y)
    # exact capacities: the guard bytes stay
    b = bufs(n, N)
    assert draw(b, n, n, N) == 0
    torch.cuda.synchronize()
    assert (b[0][n:] == 0x5A5A5A5A).all()
    for x, k in zip(b[1:], (N, N, N, 3 * N)):
        g = x[k:]
        assert (g == (0x5A5A5A5A if x.dtype == torch.int32 else 1234.5)).all()
    ref = R.rasterize(verts, faces, poses, intr, H, W, 0.1, labels, rgb)
    assert np.array_equal(b[1][:N].cpu().numpy(), ref["tri_id"].reshape(-1))
    assert np.array_equal(_bits(b[2][:N]), _bits(ref["depth"].reshape(-1)))


def test_argument_errors_raise():
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    v = torch.rand(4, 3, device="cuda")
    f = torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int32, device="cuda")
    P = torch.eye(4, device="cuda")[None]
    intr = (50.0, 50.0, 16.0, 16.0)
    ok = ops.rasterize_mesh(v, f, P, intr, 32, 32, 0.1)
    assert ok["tri_id"].shape == (1, 32, 32)
    for bad in ([[0, 1, 4]], [[0, -1, 2]]):
        with pytest.raises(UcsaError):
            ops.rasterize_mesh(v, torch.tensor(bad, dtype=torch.int32, device="cuda"), P, intr,
                               32, 32, 0.1)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v[:, :2], f, P, intr, 32, 32, 0.1)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f.view(-1), P, intr, 32, 32, 0.1)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f, P[0], intr, 32, 32, 0.1)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f, P, intr, 32, 32, 0.0)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f, P, intr, 0, 32, 0.1)
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f, P, intr, 32, 32, 0.1, vertex_labels=torch.zeros(
            3, dtype=torch.int32, device="cuda"))
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v, f, P, intr, 32, 32, 0.1, vertex_rgb=torch.zeros(4, 2, device="cuda"))
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(v.cpu(), f, P, intr, 32, 32, 0.1)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_render_mesh_labels_script_end_to_end(tmp_path, capsys):
    from scripts import render_mesh_labels as script
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    from ucsa_neural_rendering_amd.utils.semantic_mesh import ngp_to_pose_frame
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=4, H=240, W=320)
    m = ds.room.labelled_mesh(0.05)
    rgb = ds.room.palette.cpu().numpy()[m["labels"] - 1]
    mesh = str(tmp_path / "room.ply")
    write_ply(mesh, m["verts"], m["faces"], rgb=rgb, labels=m["labels"])
    out = str(tmp_path / "out")
    rec = script.main(["--scene_root", sroot, "--mesh", mesh, "--out_dir", out])
    assert rec["frames"] == 4
    stems = [f"{i:06d}" for i in range(4)]
    for s in stems:
        ml = _png(os.path.join(out, "mesh_label", s + ".png"))
        gl = _png(os.path.join(sroot, "label_40", s + ".png"))
        md = _png(os.path.join(out, "mesh_depth", s + ".png")).astype(np.float64)
        gd = _png(os.path.join(sroot, "depth", s + ".png")).astype(np.float64)
        assert ml.dtype == np.uint8 and md.shape == gd.shape == (240, 320)
        assert _png(os.path.join(out, "mesh_image", s + ".png")).shape == (240, 320, 3)
        agree = ml == gl
        # depth/ went through fp16 (half an ulp: z * 2^-11) and both sides
        # through millimetre rounding
        tol = 1.0 + gd * 2.0 ** -11
        err = np.abs(md - gd)[agree]
        with capsys.disabled():
            print(f"\n{s}: label agreement {agree.mean():.5f}, depth |err| max "
                  f"{err.max():.1f} mm, bound {tol[agree].max():.1f} mm")
        assert agree.mean() >= ROOM_AGREE_MIN
        assert (err <= tol[agree]).all()
    # the mesh written in the JSON pose frame, in metres: the same images
    mesh_pf = str(tmp_path / "room_pose_frame.ply")
    write_ply(mesh_pf, ngp_to_pose_frame(m["verts"], ds.one_m_to_scene_uom), m["faces"],
              labels=m["labels"])
    out2 = str(tmp_path / "out2")
    script.main(["--scene_root", sroot, "--mesh", mesh_pf, "--pose_frame", "--out_dir", out2])
    for s in stems:
        assert np.array_equal(_png(os.path.join(out, "mesh_label", s + ".png")),
                              _png(os.path.join(out2, "mesh_label", s + ".png")))
    # --score: pseudo-labels equal to label_40, then with permuted classes
    exp = os.path.join(sroot, "exp")
    shutil.copytree(os.path.join(sroot, "label_40"), os.path.join(exp, "nerf_label"))
    capsys.readouterr()
    rec = script.main(["--scene_root", sroot, "--mesh", mesh, "--exp_name", "exp", "--score"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["nerf_label"]["frames"] == 4 and "seg_label" not in line
    print("score, label_40 as pseudo-labels:", line["nerf_label"])
    assert rec["nerf_label"]["mIoU"] >= 0.98
    perm = np.roll(np.arange(1, 41), 7)
    from PIL import Image
    for s in stems:
        lab = _png(os.path.join(sroot, "label_40", s + ".png"))
        out_l = np.where(lab > 0, perm[np.clip(lab, 1, 40) - 1], 0).astype(np.uint8)
        Image.fromarray(out_l).save(os.path.join(exp, "nerf_label", s + ".png"))
    rec = script.main(["--scene_root", sroot, "--mesh", mesh, "--exp_name", "exp", "--score"])
    print("score, permuted classes:", rec["nerf_label"])
    assert rec["nerf_label"]["mIoU"] < 0.2
