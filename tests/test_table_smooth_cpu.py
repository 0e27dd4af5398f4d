"""CPU: neighbourhood pooling of the fused label tables.  Hand cases of the two
contracts on the numpy restatement (tests/smooth_numpy.py; the GPU kernels are
held to it bit for bit in tests/test_gpu_table_smooth.py) and the room
experiment of tests/test_evidence_cpu.py with one pooling pass.

Room set-up: exactly ``test_room_soft_fusion_is_no_worse_than_hard_votes`` (its
helpers, seed 2024: 12 fused views, 4 held out, the 96^3 volume, half of all
pixels wrong), the evidence table pooled once over 26 neighbours, resolved and
ray-cast as there.  Measured with the restatements, scored against the held-out
views' label_40:
  evidence sums:                mIoU 0.3602, accuracy 0.7981, 129753 labelled voxels
  pooled over 26 neighbours:    mIoU 0.6362, accuracy 0.9530, 157277 labelled voxels
The noise of that experiment is independent per pixel; spatially correlated
mistakes gain less."""
import os
import re

import numpy as np
import pytest

from tests import evidence_numpy as EN
from tests import smooth_numpy as SN
from tests import tsdf_numpy as TN
from tests import voxel_map_numpy as VN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_an_unobserved_voxel_neither_receives_nor_donates():
    w = np.ones((2, 2, 9), F32)
    w[0, 0, 4] = 0.5                                          # below min_weight = 1
    t = np.ones((2, 2, 2, 9), np.uint32)
    t[:, 0, 0, 4] = (1000, 2000)
    keep = t.copy()
    for nb in (6, 26):
        out = SN.smooth_voxel_table(t, w, neighbourhood=nb)
        assert out.dtype == t.dtype and out is not t and t.tobytes() == keep.tobytes()
        assert out[:, 0, 0, 4].tolist() == [1000, 2000]      # its column is copied
        assert out.max() == 2000 and (out < 1000).sum() == out.size - 2   # it donates nothing
        # its face neighbour along z: itself, (0,0,2), (1,0,3), (0,1,3); with the cube also
        # (1,1,3) and the three other voxels of each of the slabs z = 2 and z = 4
        assert out[0, 0, 0, 3] == (4 if nb == 6 else 11) and out[1, 0, 0, 5] == out[0, 0, 0, 3]
        assert out[0, 1, 1, 4] == (5 if nb == 6 else 11)      # a diagonal neighbour of it
        assert out[0, 1, 1, 0] == (4 if nb == 6 else 8)       # a corner of the lattice
    # min_weight moves the gate, NaN is never observed
    assert SN.smooth_voxel_table(t, w, min_weight=0.5)[0, 0, 0, 4] == 1000 + 11
    w[:] = np.nan
    assert SN.smooth_voxel_table(t, w).tobytes() == t.tobytes()


def test_taps_inside_the_lattice_the_centre_weight_and_both_neighbourhoods():
    w = np.ones((3, 3, 3), F32)
    t = np.ones((3, 3, 3, 3), np.uint16)
    out = SN.smooth_voxel_table(t, w, neighbourhood=26)
    assert out.dtype == np.uint16
    # a corner has 7 neighbours inside, an edge 11, a face 17, the middle 26
    assert out[0, 0, 0, 0] == 8 and out[1, 1, 0, 0] == 12 and out[2, 1, 1, 0] == 18
    assert out[0, 1, 1, 1] == 27
    out = SN.smooth_voxel_table(t, w, neighbourhood=6)
    assert out[0, 0, 0, 0] == 4 and out[1, 1, 0, 0] == 5 and out[2, 1, 1, 0] == 6
    assert out[0, 1, 1, 1] == 7
    out = SN.smooth_voxel_table(t, w, neighbourhood=26, centre=3)
    assert out[0, 0, 0, 0] == 10 and out[0, 1, 1, 1] == 29
    # a single spike spreads to the cube around it, weighted 3 at home
    t[:] = 0
    t[1, 1, 1, 1] = 5
    out = SN.smooth_voxel_table(t, w, neighbourhood=6, centre=3)
    assert out[1, 1, 1, 1] == 15 and out[1].sum() == 15 + 6 * 5 and not out[[0, 2]].any()
    assert out[1, 0, 1, 1] == 5 and out[1, 0, 0, 1] == 0
    for bad in (dict(neighbourhood=18), dict(centre=0), dict(centre=256), dict(iterations=0)):
        with pytest.raises(ValueError):
            SN.smooth_voxel_table(t, w, **bad)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint16])
def test_sums_saturate(dtype):
    sat = SN.SAT[np.dtype(dtype)]
    w = np.ones((3, 3, 3), F32)
    t = np.full((2, 3, 3, 3), sat - 30, dtype)
    out = SN.smooth_voxel_table(t, w)
    assert out.dtype == dtype and (out == sat).all()
    # exact below the limit: sat - 27 spread as ones
    t[:] = 0
    t[0, 1, 1, 1] = sat - 27
    t[1] = 1
    t[1, 1, 1, 1] = sat - 26
    out = SN.smooth_voxel_table(t, w)
    assert out[0, 1, 1, 1] == sat - 27 and out[1, 1, 1, 1] == sat and out[1, 0, 0, 0] == sat - 19
    assert SN.smooth_voxel_table(t, w, centre=255)[0, 1, 1, 1] == sat


def test_two_iterations_are_two_calls():
    g = np.random.default_rng(1)
    w = (g.random((5, 4, 7)) < 0.6).astype(F32)
    t = g.integers(0, 1000, (4, 5, 4, 7)).astype(np.uint32)
    for nb in (6, 26):
        once = SN.smooth_voxel_table(t, w, neighbourhood=nb, centre=2)
        twice = SN.smooth_voxel_table(once, w, neighbourhood=nb, centre=2)
        both = SN.smooth_voxel_table(t, w, neighbourhood=nb, centre=2, iterations=2)
        assert both.tobytes() == twice.tobytes() and both.tobytes() != once.tobytes()
        assert (once[:, w < 1] == t[:, w < 1]).all()


def test_mesh_fan_isolated_duplicated_and_degenerate_faces():
    # a fan around vertex 0 over the rim 1..5, face (0,1,2) listed twice, a face
    # with a repeated vertex (it gives its proper edge 5-7 alone), a face that is one
    # point, vertex 6 isolated
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 1, 2], [5, 5, 7],
                      [3, 3, 3]], np.int32)
    off, nbr = SN.mesh_adjacency(faces, 8)
    assert off.dtype == np.int32 and nbr.dtype == np.int32
    assert off.tolist() == [0, 5, 7, 10, 13, 16, 19, 19, 20]
    rows = [nbr[off[v]:off[v + 1]].tolist() for v in range(8)]
    assert rows == [[1, 2, 3, 4, 5], [0, 2], [0, 1, 3], [0, 2, 4], [0, 3, 5], [0, 4, 7], [], [5]]
    votes = np.zeros((8, 3), np.uint64)
    votes[:, 0] = 1
    votes[:, 1] = 10 ** np.arange(8)
    votes[6, 2] = 7
    out = SN.smooth_label_table(votes, (off, nbr), centre=3)
    assert out.dtype == np.uint64 and out is not votes and votes[0, 1] == 1
    assert out[:, 0].tolist() == [8, 5, 6, 6, 6, 6, 3, 4]    # centre + degree
    assert out[0, 1] == 111113 and out[6].tolist() == [3, 3000000, 21]
    assert out[7, 1] == 30000000 + 100000 and out[5, 1] == 300000 + 1 + 10000 + 10000000
    # modulo 2^64
    votes[1, 2] = votes[2, 2] = 2 ** 63
    assert SN.smooth_label_table(votes, (off, nbr))[0, 2] == 0
    once = SN.smooth_label_table(votes, (off, nbr), centre=2)
    assert SN.smooth_label_table(votes, (off, nbr), iterations=2, centre=2).tobytes() == \
        SN.smooth_label_table(once, (off, nbr), centre=2).tobytes()


def test_room_one_pooling_pass_lifts_the_soft_fusion():
    from tests.test_evidence_cpu import noisy_beliefs
    from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec
    from tests.test_voxel_map_cpu import ROOM_FAR, ROOM_NEAR, room_labels, score
    H, W, C = 120, 160, 40
    room, poses, intr, depth = room_frames(H, W)
    truth = room_labels(room, poses, intr, depth)
    held = np.arange(16) % 4 == 3
    dims, origin, h, trunc = room_volume_spec(96)
    vol = TN.new_volume(dims, origin, h)
    TN.integrate(vol, depth[~held], poses[~held], intr, trunc)
    p, top = noisy_beliefs(truth[~held], C, seed=2024)
    ev = EN.accumulate(EN.new_evidence(dims, C), vol, depth[~held], EN.log_evidence(p),
                       poses[~held], intr, trunc)
    pooled = SN.smooth_voxel_table(ev, vol["weight"], neighbourhood=26, iterations=1)
    res, count = {}, {}
    for name, table in (("unsmoothed", ev), ("26 / 1", pooled)):
        lab = EN.resolve(table)[0]
        count[name] = int((lab > 0).sum())
        out = VN.raycast(vol, poses[held], intr, H, W, ROOM_NEAR, ROOM_FAR, trunc,
                         step=0.5 * float(h), voxel_labels=lab, skip=True)
        res[name] = score(out["label"], truth[held])
        print(f"{name}: mIoU {res[name]['mIoU']:.4f}, accuracy {res[name]['total_acc']:.4f}, "
              f"{count[name]} labelled voxels")
    assert res["26 / 1"]["total_acc"] >= 0.93
    assert res["26 / 1"]["mIoU"] >= 0.61
    assert count["26 / 1"] > count["unsmoothed"]


def test_entries_are_declared_and_bound():
    from ucsa_neural_rendering_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "ucsa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("ucsa_voxel_table_smooth", 12), ("ucsa_label_table_smooth", 9)):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
        assert callable(getattr(_lib.lib(), name))
    for f in ("smooth_voxel_table", "mesh_adjacency", "smooth_label_table"):
        assert callable(getattr(ops, f)), f
    # argument errors come before anything touches a device
    l = _lib.lib()
    assert l.ucsa_voxel_table_smooth(None, None, 4, 40, 8, 8, 8, None, 1.0, 26, 1, None) == -1000
    assert l.ucsa_label_table_smooth(None, None, 5, 0, None, None, 0, 1, None) == -1003
    import inspect
    from scripts import fuse_mesh_labels, voxel_map_labels
    from ucsa_neural_rendering_amd.utils import mesh_fusion, voxel_map
    sig = inspect.signature(voxel_map.fuse_semantic_views).parameters
    assert sig["smooth"].default == 0 and sig["smooth_neighbourhood"].default == 26
    assert inspect.signature(mesh_fusion.fuse_views).parameters["smooth"].default == 0
    for mod in (voxel_map_labels, fuse_mesh_labels):
        tail = ["--out_dir", "o"] if mod is voxel_map_labels else ["--mesh", "m.ply", "--out",
                                                                   "o.ply"]
        base = ["--scene_root", "s", "--labels", "label_40"] + tail
        assert mod.parse_args(base).smooth == 0
        assert mod.parse_args(base + ["--smooth", "2"]).smooth == 2
    a = voxel_map_labels.parse_args(base[:4] + ["--out_dir", "o", "--smooth", "1",
                                                "--smooth_neighbourhood", "6"])
    assert a.smooth_neighbourhood == 6
    assert voxel_map_labels.parse_args(base[:4] + ["--out_dir", "o"]).smooth_neighbourhood == 26
    with pytest.raises(SystemExit):
        voxel_map_labels.parse_args(base[:4] + ["--out_dir", "o", "--smooth_neighbourhood", "18"])
