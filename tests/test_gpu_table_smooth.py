"""GPU: neighbourhood pooling of the fused label tables (k_voxel_smooth and
k_label_smooth of csrc/table_smooth.hip, ops.mesh_adjacency) against the numpy
restatement of their contracts (tests/smooth_numpy.py).  Every comparison is
byte equality.  Both scripts with --smooth on an exported synthetic scene with
noisy inputs (half of all pixels wrong, independently per pixel)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import smooth_numpy as SN
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
# odd sizes over several tiles of 4 x 4 x 64; a volume smaller than one tile; a thin axis
LATTICES = [(37, 20, 65), (2, 2, 9), (5, 70, 3)]
NP_DTYPE = {torch.uint32: np.uint32, torch.uint16: np.uint16}


def lattice_case(dims, n_classes, dtype, observed, seed=0):
    """a table of small random values with a slab within 30 of SAT, and weights
    with about ``observed`` of the voxels at or above 1"""
    g = np.random.default_rng(seed + 7 * n_classes + dims[0])
    sat = SN.SAT[np.dtype(dtype)]
    t = g.integers(0, 2000, (n_classes + 1,) + dims).astype(dtype)
    slab = (slice(None), slice(0, 2), slice(None), slice(dims[2] // 2, dims[2] // 2 + 3))
    t[slab] = (sat - g.integers(0, 31, t[slab].shape)).astype(dtype)
    w = np.where(g.random(dims) < observed, g.uniform(1.0, 9.0, dims), g.uniform(0.0, 0.99, dims))
    w = w.astype(F32)
    if 0.0 < observed < 1.0:
        w.reshape(-1)[::17] = np.nan                         # never observed
        w.reshape(-1)[5::23] = 1.0                           # exactly at the threshold
    return t, w


def gpu_volume(w):
    return {"tsdf": torch.ones(w.shape, device="cuda"), "weight": _cu(w), "rgb": None,
            "origin": (0.0, 0.0, 0.0), "spacing": (1.0, 1.0, 1.0)}


@pytest.mark.parametrize("dtype", [torch.uint32, torch.uint16])
@pytest.mark.parametrize("dims,n_classes", [(d, c) for d in LATTICES for c in (1, 5, 40)] +
                         [((2, 2, 9), 255)])
def test_lattice_bit_exact_for_both_neighbourhoods_and_centres(dims, n_classes, dtype):
    ops = _ops()
    t, w = lattice_case(dims, n_classes, NP_DTYPE[dtype], 0.6)
    assert 0.3 < (w >= 1).mean() < 0.9 or w.size < 100
    vol, table = gpu_volume(w), _cu(t)
    for nb in (6, 26):
        for centre in (1, 3):
            got = ops.smooth_voxel_table(table, vol, neighbourhood=nb, centre=centre)
            want = SN.smooth_voxel_table(t, w, neighbourhood=nb, centre=centre)
            assert got.dtype == dtype and tuple(got.shape) == t.shape
            assert got.data_ptr() != table.data_ptr()
            assert got.cpu().numpy().tobytes() == want.tobytes(), (nb, centre)
            assert (want == SN.SAT[want.dtype]).any() or n_classes == 255
    assert table.cpu().numpy().tobytes() == t.tobytes()      # the input is untouched


@pytest.mark.parametrize("dtype", [torch.uint32, torch.uint16])
@pytest.mark.parametrize("dims", LATTICES)
def test_lattice_all_observed_none_observed_min_weight_and_iterations(dims, dtype):
    ops = _ops()
    for observed, nb, centre in ((1.0, 26, 1), (1.0, 6, 3), (0.0, 26, 1), (0.0, 6, 3)):
        t, w = lattice_case(dims, 5, NP_DTYPE[dtype], observed, seed=1)
        got = ops.smooth_voxel_table(_cu(t), gpu_volume(w), neighbourhood=nb, centre=centre)
        want = SN.smooth_voxel_table(t, w, neighbourhood=nb, centre=centre)
        assert got.cpu().numpy().tobytes() == want.tobytes(), (observed, nb, centre)
        if observed == 0.0:
            assert got.cpu().numpy().tobytes() == t.tobytes()
    t, w = lattice_case(dims, 5, NP_DTYPE[dtype], 0.6, seed=2)
    vol, table = gpu_volume(w), _cu(t)
    got = ops.smooth_voxel_table(table, vol, min_weight=4.0)
    assert got.cpu().numpy().tobytes() == SN.smooth_voxel_table(t, w, min_weight=4.0).tobytes()
    for nb in (6, 26):
        once = ops.smooth_voxel_table(table, vol, neighbourhood=nb, centre=2)
        twice = ops.smooth_voxel_table(once, vol, neighbourhood=nb, centre=2)
        both = ops.smooth_voxel_table(table, vol, neighbourhood=nb, centre=2, iterations=2)
        three = ops.smooth_voxel_table(table, vol, neighbourhood=nb, centre=2, iterations=3)
        assert torch.equal(both, twice) and not torch.equal(both, once)
        want = SN.smooth_voxel_table(t, w, neighbourhood=nb, centre=2, iterations=3)
        assert three.cpu().numpy().tobytes() == want.tobytes()
    assert table.cpu().numpy().tobytes() == t.tobytes()


@pytest.mark.parametrize("dtype", [torch.uint32, torch.uint16])
def test_lattice_writes_nothing_outside_its_output_and_rejects_bad_arguments(dtype):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    dims, Cn = (5, 70, 3), 5
    t, w = lattice_case(dims, Cn, NP_DTYPE[dtype], 0.6, seed=3)
    n = int(np.prod(dims))
    src, check_src = guarded(t.shape, dtype, 0)
    src.copy_(_cu(t))
    dst, check_dst = guarded(t.shape, dtype, 0)
    wt, check_w = guarded(dims, torch.float32, 0.0)
    wt.copy_(_cu(w))
    l = _lib.lib()
    p = lambda x: C.c_void_p(x.data_ptr())

    def call(a, b, es=t.itemsize, cn=Cn, d=dims, wp=None, mw=1.0, nb=26, centre=1):
        return l.ucsa_voxel_table_smooth(a, b, es, cn, d[0], d[1], d[2], wp or p(wt), mw, nb,
                                         centre, None)
    torch.cuda.synchronize()
    assert call(p(src), p(dst)) == 0
    torch.cuda.synchronize()
    for chk in (check_src, check_dst, check_w):
        chk()
    assert dst.cpu().numpy().tobytes() == SN.smooth_voxel_table(t, w).tobytes()
    assert src.cpu().numpy().tobytes() == t.tobytes()
    # argument errors: code = -(1000 + argument), nothing is launched, nothing written
    before = dst.clone()
    inside = C.c_void_p(src.data_ptr() + t.itemsize * (t.size - 1))
    for rc, want in ((call(p(src), p(src)), 1), (call(p(src), inside), 1),
                     (call(p(src), p(wt)), 1), (call(None, p(dst)), 0), (call(p(src), None), 1),
                     (call(p(src), p(dst), es=8), 2), (call(p(src), p(dst), cn=0), 3),
                     (call(p(src), p(dst), cn=256), 3), (call(p(src), p(dst), d=(1, 70, 3)), 4),
                     (call(p(src), p(dst), d=(5, 1, 3)), 5), (call(p(src), p(dst), d=(5, 70, 1)), 6),
                     (call(p(src), p(dst), mw=float("nan")), 8), (call(p(src), p(dst), nb=18), 9),
                     (call(p(src), p(dst), centre=0), 10), (call(p(src), p(dst), centre=256), 10)):
        assert rc == -(1000 + want), (rc, want)
    torch.cuda.synchronize()
    assert torch.equal(dst, before) and src.cpu().numpy().tobytes() == t.tobytes()
    vol = gpu_volume(w)
    for bad in (lambda: ops.smooth_voxel_table(_cu(t).view(torch.int16 if t.itemsize == 2
                                                           else torch.int32), vol),
                lambda: ops.smooth_voxel_table(_cu(t)[:, :, :-1], vol),
                lambda: ops.smooth_voxel_table(_cu(t)[:, :, :-1].contiguous(), vol),
                lambda: ops.smooth_voxel_table(_cu(t)[0], vol),
                lambda: ops.smooth_voxel_table(torch.from_numpy(t), vol),
                lambda: ops.smooth_voxel_table(_cu(t), vol, neighbourhood=18),
                lambda: ops.smooth_voxel_table(_cu(t), vol, centre=0),
                lambda: ops.smooth_voxel_table(_cu(t), vol, centre=1.5),
                lambda: ops.smooth_voxel_table(_cu(t), vol, iterations=0)):
        with pytest.raises(_lib.UcsaError):
            bad()


V_MESH = 500


def mesh_faces(seed=4):
    """random faces over vertices 0..449 (450..499 stay isolated), a hub (vertex
    0) with a fan of 320 faces, faces listed twice and degenerate faces"""
    g = np.random.default_rng(seed)
    rnd = g.integers(1, 450, (700, 3))
    fan = np.stack([np.zeros(320, np.int64), np.arange(1, 321), np.arange(2, 322)], 1)
    degenerate = np.array([[7, 7, 9], [11, 12, 11], [13, 13, 13], [460, 460, 460]])
    faces = np.concatenate([rnd, fan, rnd[:40], fan[5:9, ::-1], degenerate]).astype(np.int32)
    return faces[g.permutation(faces.shape[0])]


@pytest.mark.parametrize("n_classes", [1, 40, 255])
def test_mesh_adjacency_and_table_bit_exact(n_classes):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    faces = mesh_faces()
    want_off, want_nbr = SN.mesh_adjacency(faces, V_MESH)
    deg = np.diff(want_off)
    assert deg[0] >= 300 and (deg[450:] == 0).all() and deg[460] == 0
    off, nbr = ops.mesh_adjacency(_cu(faces), V_MESH)
    assert off.dtype == torch.int32 and nbr.dtype == torch.int32
    assert off.cpu().numpy().tobytes() == want_off.tobytes()
    assert nbr.cpu().numpy().tobytes() == want_nbr.tobytes()
    g = np.random.default_rng(n_classes)
    votes = g.integers(0, 2 ** 64, (V_MESH, n_classes + 1), dtype=np.uint64)   # sums wrap
    votes[100:200] = g.integers(0, 1000, (100, n_classes + 1))
    table, check = guarded(votes.shape, torch.int64, 0)
    table.copy_(_cu(votes.view(np.int64)))
    for centre, it in ((1, 1), (3, 1), (2, 2)):
        got = ops.smooth_label_table(table, (off, nbr), iterations=it, centre=centre)
        want = SN.smooth_label_table(votes, (want_off, want_nbr), iterations=it, centre=centre)
        assert got.dtype == torch.int64 and got.data_ptr() != table.data_ptr()
        assert got.cpu().numpy().view(np.uint64).tobytes() == want.tobytes(), (centre, it)
    once = ops.smooth_label_table(table, (off, nbr), centre=2)
    assert torch.equal(ops.smooth_label_table(once, (off, nbr), centre=2), got)
    torch.cuda.synchronize()
    check()
    assert table.cpu().numpy().view(np.uint64).tobytes() == votes.tobytes()
    # degree 0: centre * votes[v]
    assert (got[470].cpu().numpy().view(np.uint64) ==
            votes[470] * np.uint64(4)).all()
    # aliased and mis-shaped arguments
    l = _lib.lib()
    p = lambda x: C.c_void_p(x.data_ptr())
    out = torch.zeros_like(table)
    E = nbr.numel()
    assert l.ucsa_label_table_smooth(p(table), p(table), V_MESH, n_classes, p(off), p(nbr), E, 1,
                                     None) == -1001
    assert l.ucsa_label_table_smooth(p(table), p(out), V_MESH, 0, p(off), p(nbr), E, 1,
                                     None) == -1003
    assert l.ucsa_label_table_smooth(p(table), p(out), V_MESH, n_classes, p(off), p(nbr), E, 0,
                                     None) == -1007
    assert l.ucsa_label_table_smooth(p(table), p(out), V_MESH, n_classes, None, p(nbr), E, 1,
                                     None) == -1004
    torch.cuda.synchronize()
    assert not out.any()
    for bad in (lambda: ops.smooth_label_table(table, (off[:-1], nbr)),
                lambda: ops.smooth_label_table(table, (off.long(), nbr)),
                lambda: ops.smooth_label_table(table, off),
                lambda: ops.smooth_label_table(table.view(torch.float64), (off, nbr)),
                lambda: ops.smooth_label_table(table, (off, nbr), centre=256),
                lambda: ops.smooth_label_table(table, (off, nbr), iterations=0),
                lambda: ops.mesh_adjacency(_cu(faces).long(), V_MESH),
                lambda: ops.mesh_adjacency(_cu(faces), 400)):
        with pytest.raises(_lib.UcsaError):
            bad()


def test_scripts_with_smooth_fill_and_improve_noisy_inputs(tmp_path):
    """The scene and sizes of tests/test_gpu_evidence.py's script test; beliefs
    as in the room experiment (tests/test_evidence_cpu.noisy_beliefs: the argmax
    wrong with probability 0.5, independently per pixel)."""
    import os

    from PIL import Image

    from scripts import fuse_mesh_labels, voxel_map_labels
    from tests.test_evidence_cpu import noisy_beliefs
    from tests.test_gpu_evidence import _png
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    ops = _ops()
    Hs, Ws, n, Cn = 240, 320, 8, 40
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=Hs, W=Ws)
    stems = [f"{b:06d}" for b in range(n)]
    truth = np.stack([_png(os.path.join(sroot, "label_40", s + ".png")) for s in stems])
    p, top = noisy_beliefs(truth, Cn, seed=7)
    os.makedirs(tmp_path / "codes")
    os.makedirs(tmp_path / "noisy")
    for b, s in enumerate(stems):
        codes = ops.log_evidence(_cu(p[b:b + 1]))[0].cpu().numpy()
        np.save(tmp_path / "codes" / (s + ".npy"), codes)
        Image.fromarray((top[b] + 1).astype(np.uint8)).save(tmp_path / "noisy" / (s + ".png"))

    def labelled(folder):
        return sum(int((_png(os.path.join(folder, "map_label", s + ".png")) > 0).sum())
                   for s in stems)

    h = 6.1 / 63
    common = ["--scene_root", sroot, "--voxel", repr(h), "--step", repr(0.5 * h), "--aabb",
              "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05", "--score", "--scores",
              str(tmp_path / "codes")]
    today = voxel_map_labels.main(common + ["--out_dir", str(tmp_path / "v")])
    zero = voxel_map_labels.main(common + ["--smooth", "0", "--out_dir", str(tmp_path / "v0")])
    one = voxel_map_labels.main(common + ["--smooth", "1", "--out_dir", str(tmp_path / "v1")])
    six = voxel_map_labels.main(common + ["--smooth", "1", "--smooth_neighbourhood", "6",
                                          "--out_dir", str(tmp_path / "v6")])
    assert "smooth" not in zero and one["smooth"] == [1, 26] and six["smooth"] == [1, 6]
    for s in stems:
        for k in ("map_label", "map_depth"):
            assert _png(tmp_path / "v0" / k / (s + ".png")).tobytes() == \
                _png(tmp_path / "v" / k / (s + ".png")).tobytes(), (k, s)
    assert zero["voxel_map"] == today["voxel_map"] and zero["labelled"] == today["labelled"]
    print("voxel map:", today["voxel_map"], one["voxel_map"], six["voxel_map"],
          labelled(tmp_path / "v"), labelled(tmp_path / "v1"))
    for rec, folder in ((one, "v1"), (six, "v6")):
        assert labelled(tmp_path / folder) >= labelled(tmp_path / "v") > 0
        assert rec["labelled"] >= today["labelled"]
        assert rec["voxel_map"]["mIoU"] >= today["voxel_map"]["mIoU"]
        assert rec["voxel_map"]["total_acc"] >= today["voxel_map"]["total_acc"]
    # the mesh route, on the hard noisy labels
    m = ds.room.labelled_mesh(0.1)
    mesh = str(tmp_path / "room_geometry.ply")
    write_ply(mesh, m["verts"], m["faces"])
    args = ["--scene_root", sroot, "--mesh", mesh, "--labels", str(tmp_path / "noisy"), "--score"]
    rt = fuse_mesh_labels.main(args + ["--out", str(tmp_path / "t.ply"), "--out_dir",
                                       str(tmp_path / "m")])
    r0 = fuse_mesh_labels.main(args + ["--smooth", "0", "--out", str(tmp_path / "0.ply"),
                                       "--out_dir", str(tmp_path / "m0")])
    r1 = fuse_mesh_labels.main(args + ["--smooth", "1", "--out", str(tmp_path / "1.ply"),
                                       "--out_dir", str(tmp_path / "m1")])
    assert open(tmp_path / "0.ply", "rb").read() == open(tmp_path / "t.ply", "rb").read()
    for s in stems:
        assert _png(tmp_path / "m0" / "map_label" / (s + ".png")).tobytes() == \
            _png(tmp_path / "m" / "map_label" / (s + ".png")).tobytes(), s
    print("mesh:", rt["fused"], r1["fused"], labelled(tmp_path / "m"), labelled(tmp_path / "m1"))
    assert "smooth" not in r0 and r1["smooth"] == 1 and r0["fused"] == rt["fused"]
    assert r1["observed"] >= rt["observed"] > 0
    assert labelled(tmp_path / "m1") >= labelled(tmp_path / "m") > 0
    assert r1["fused"]["mIoU"] >= rt["fused"]["mIoU"]
    assert r1["fused"]["total_acc"] >= rt["fused"]["total_acc"]
