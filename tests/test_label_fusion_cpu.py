"""CPU: the numpy restatement of the label-fusion contract
(tests/fusion_numpy.py), which the GPU tables are held to bit for bit, and the
fusion scheme itself on the analytic room with the numpy rasterizer.

- Properties of the restatement: order independence, split calls, the tie and
  min_votes rules, ignored ids / classes, the depth gate (NaN, sensor = 0),
  weights.
- The two C entries are declared in the header and in the ctypes table.
- The room: votes taken from the mesh's own clean label render reproduce the
  mesh's labels on every observed vertex; with per-view label noise, the fused
  mesh rendered into held-out views agrees with the clean render better than
  the noisy input does."""
import os
import re

import numpy as np
import pytest

from tests import fusion_numpy as FN
from tests import raster_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_votes(seed, n, V, C):
    g = np.random.default_rng(seed)
    vid = g.integers(-2, V + 3, n).astype(np.int32)
    pred = g.integers(0, C + 4, n).astype(np.uint8)
    w = g.integers(-3, 65540, n).astype(np.int32)
    w[::7] = 65535
    w[1::7] = 0
    md = g.uniform(0.5, 5.0, n).astype(np.float32)
    sd = (md + g.normal(0, 0.02, n)).astype(np.float32)
    sd[::11] = 0.0
    sd[3::13] = np.nan
    md[5::17] = np.nan
    return vid, pred, w, md, sd


def test_order_and_grouping_do_not_matter():
    V, C = 37, 40
    vid, pred, w, md, sd = _random_votes(0, 20000, V, C)
    kw = dict(weight=w, mesh_depth=md, sensor_depth=sd, depth_tol=0.03)
    one = FN.accumulate(FN.new_table(V, C), vid, pred, **kw)
    assert one.sum() > 0
    p = np.random.default_rng(1).permutation(vid.size)
    shuffled = FN.accumulate(FN.new_table(V, C), vid[p], pred[p], weight=w[p], mesh_depth=md[p],
                             sensor_depth=sd[p], depth_tol=0.03)
    assert np.array_equal(one, shuffled)
    parts = FN.new_table(V, C)
    for a, b in ((0, 1), (1, 7001), (7001, 7001), (7001, 20000)):
        FN.accumulate(parts, vid[a:b], pred[a:b], weight=w[a:b], mesh_depth=md[a:b],
                      sensor_depth=sd[a:b], depth_tol=0.03)
    assert np.array_equal(one, parts)
    assert (one[:, 0] == 0).all()


def test_ids_and_classes_outside_their_range_are_ignored():
    V, C = 3, 5
    vid = np.array([0, -1, 4, 1, 1, 3, 3, 2], np.int32)
    pred = np.array([1, 1, 1, 0, 6, 5, 255, 2], np.uint8)
    t = FN.accumulate(FN.new_table(V, C), vid, pred)
    want = FN.new_table(V, C)
    want[2, 5] = 1
    want[1, 2] = 1
    assert np.array_equal(t, want)


def test_weights_add_and_out_of_range_weights_do_not_vote():
    V, C = 2, 3
    vid = np.array([1, 1, 1, 2, 2, 2], np.int32)
    pred = np.array([2, 2, 3, 1, 1, 1], np.uint8)
    w = np.array([65535, 65535, 0, -1, 65536, 7], np.int32)
    t = FN.accumulate(FN.new_table(V, C), vid, pred, weight=w)
    assert t[0, 2] == 2 * 65535 and t[0, 3] == 0 and t[1, 1] == 7 and t.sum() == 2 * 65535 + 7
    # the table is uint64: a cell can pass 2^32
    big = FN.new_table(1, 1)
    n = 70000
    FN.accumulate(big, np.ones(n, np.int32), np.ones(n, np.uint8), weight=np.full(n, 65535))
    assert int(big[0, 1]) == n * 65535 > 2 ** 32


def test_depth_gate():
    V, C = 1, 2
    md = np.array([1.0, 1.0, 1.0, 1.0, np.nan, 1.0, 1.0, 1.0], np.float32)
    sd = np.array([1.0, 1.05, 0.95, 1.2, 1.0, np.nan, 0.0, -1.0], np.float32)
    vid = np.ones(8, np.int32)
    pred = np.ones(8, np.uint8)
    tol = np.float32(0.05)
    t = FN.accumulate(FN.new_table(V, C), vid, pred, mesh_depth=md, sensor_depth=sd, depth_tol=tol)
    # one fp32 subtraction decides: |1 - 1.05f| and |1 - 0.95f| against 0.05f
    keep = (sd > 0) & (np.abs(md - sd) <= tol)
    assert keep[0] and not keep[3:].any()
    assert int(t[0, 1]) == int(keep.sum())
    with pytest.raises(ValueError):
        FN.accumulate(FN.new_table(V, C), vid, pred, mesh_depth=md)


def test_resolve_ties_min_votes_and_winner():
    t = FN.new_table(5, 4)
    t[0, 1:] = [3, 7, 7, 1]   # tie: the lower class
    t[1, 1:] = [0, 0, 0, 2]
    t[2, 1:] = [0, 0, 0, 0]   # unobserved
    t[3, 1:] = [1, 1, 1, 1]
    t[4, 1:] = [0, 2 ** 40, 5, 0]
    t[:, 0] = 99              # column 0 is never read
    label, total, winner = FN.resolve(t)
    assert label.tolist() == [2, 4, 0, 1, 2] and label.dtype == np.int32
    assert total.tolist() == [18, 2, 0, 4, 2 ** 40 + 5] and total.dtype == np.uint64
    assert winner.tolist() == [7, 2, 0, 1, 2 ** 40]
    label3, total3, winner3 = FN.resolve(t, min_votes=3)
    assert label3.tolist() == [2, 0, 0, 1, 2]
    assert np.array_equal(total3, total) and np.array_equal(winner3, winner)
    e = FN.resolve(FN.new_table(0, 4))
    assert all(x.shape == (0,) for x in e)


def test_entries_are_declared_and_bound():
    from ucsa_neural_rendering_amd import _lib
    src = open(os.path.join(ROOT, "include", "ucsa_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("ucsa_label_fuse_accumulate", "ucsa_label_fuse_resolve"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ucsa_label_fuse_accumulate"][1]) == 14
    assert len(_lib.SIGNATURES["ucsa_label_fuse_resolve"][1]) == 9
    from ucsa_neural_rendering_amd import ops
    assert callable(ops.fuse_label_votes) and callable(ops.resolve_label_votes)


# ---- the scheme on the analytic room -------------------------------------
ROOM_STEP, ROOM_H, ROOM_W = 0.1, 120, 160
HELD_OUT = (3, 7, 11, 15)
NOISE_P, NOISE_SEED = 0.5, 2024
# Measured with this restatement for (step 0.1, 120x160, p = 0.5, seed 2024,
# 12 fused + 4 held-out views of _slerp_loop_poses(16, seed=123)); the GPU path
# is bit-identical to the restatement, so they hold for it too:
#   input accuracy (held-out views)            0.5096   (fused views 0.5126)
#   share of vertices observed                 0.4890   (23 855 vertices)
#   vertex accuracy over observed vertices     0.9865
#   held-out agreement with the clean render   0.9653
#   held-out pixels left unlabelled            0.0305
# Floor: 0.01 below the measured agreement (the run is seeded and integer from
# the votes on; the margin only covers another numpy's random stream).
HELD_OUT_AGREE_MIN = 0.9553
# a condition, not a result: pixels of the held-out views on unobserved vertices
UNLABELLED_MAX = 0.05


def room_setup():
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom, \
        _slerp_loop_poses
    m = SyntheticRoom(0).labelled_mesh(ROOM_STEP)
    poses = _slerp_loop_poses(16, seed=123).numpy()
    intr = (0.89 * ROOM_W, 0.89 * ROOM_W, ROOM_W / 2.0, ROOM_H / 2.0)
    fused = [i for i in range(16) if i not in HELD_OUT]
    return m, poses, intr, fused, list(HELD_OUT)


def noisy_labels(clean, p=NOISE_P, seed=NOISE_SEED):
    """every covered pixel replaced by a uniformly random class with probability
    p, independently per view and pixel"""
    g = np.random.default_rng(seed)
    flip = g.random(clean.shape) < p
    out = clean.copy()
    out[flip] = g.integers(1, 41, int(flip.sum()))
    return np.where(clean > 0, out, 0).astype(np.uint8)


@pytest.fixture(scope="module")
def room_case():
    m, poses, intr, fused, held = room_setup()
    clean = R.rasterize(m["verts"], m["faces"], poses, intr, ROOM_H, ROOM_W, 0.05,
                        m["labels"])["label"]
    return m, poses, intr, fused, held, clean


def test_clean_votes_reproduce_the_mesh_labels_exactly(room_case):
    m, poses, intr, fused, held, clean = room_case
    out = FN.fuse_views(m, poses[fused], intr, ROOM_H, ROOM_W, 0.05,
                        clean[fused].astype(np.uint8))
    obs = out["labels"] > 0
    assert obs.sum() == out["observed"] > 0.4 * obs.size
    assert np.array_equal(out["labels"][obs], m["labels"][obs])
    # one class per vertex: every vote of a row sits in one cell
    assert np.array_equal(out["winner"], out["total"])
    assert (out["total"][~obs] == 0).all()


def test_fusion_beats_its_noisy_input_on_held_out_views(room_case):
    m, poses, intr, fused, held, clean = room_case
    noisy = noisy_labels(clean)
    out = FN.fuse_views(m, poses[fused], intr, ROOM_H, ROOM_W, 0.05, noisy[fused])
    obs = out["labels"] > 0
    vertex_acc = (out["labels"][obs] == m["labels"][obs]).mean()
    rend = R.rasterize(m["verts"], m["faces"], poses[held], intr, ROOM_H, ROOM_W, 0.05,
                       out["labels"])["label"]
    cov = clean[held] > 0
    input_acc = (noisy[held][cov] == clean[held][cov]).mean()
    agree = (rend[cov] == clean[held][cov]).mean()
    unlabelled = (rend[cov] == 0).mean()
    print(f"input accuracy {input_acc:.4f}, observed {obs.mean():.4f}, vertex accuracy "
          f"{vertex_acc:.4f}, held-out agreement {agree:.4f}, unlabelled {unlabelled:.4f}")
    assert unlabelled <= UNLABELLED_MAX
    assert agree > input_acc
    assert agree >= HELD_OUT_AGREE_MIN
