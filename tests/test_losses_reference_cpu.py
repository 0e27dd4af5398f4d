"""tests/losses_numpy.py, the float64 yardstick of the loss / post-processing /
metric / Adam kernels, held against the oracle (oracle/losses.py), the torch
modules the reference configures and float64 autograd, against the committed
fixtures, and a few hand-computed values.  The same formulas in the same
precision: agreement at 1e-12 relative.  No GPU, no HIP library."""
import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import losses_numpy as LN
from tests.util import load_golden

REL = 1e-12
W_SEM, W_DEPTH = ol.WEIGHT_SEMANTICS, ol.WEIGHT_DEPTH


def _close(a, b, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return
    s = float(np.abs(b[ok]).max()) if scale is None else scale
    assert float(np.abs(a[ok] - b[ok]).max()) <= REL * max(s, 1e-300)


def _rows_close(a, b, floor):
    """Row by row, relative to the row's own largest entry (a row whose label
    has probability 0 is ~1e12 times the others and must not hide them)."""
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    tol = REL * np.maximum(np.abs(b).max(axis=1), floor)
    assert np.all(np.abs(a - b).max(axis=1) <= tol)


@pytest.mark.parametrize("N,C,kind", [(n, c, "plain") for n, c in LN.NERF_SHAPES] + LN.NERF_SPECIAL)
def test_nerf_loss_ref_is_the_oracle_in_float64(N, C, kind):
    case = LN.nerf_case(N, C, kind)
    stats, grads = LN.nerf_loss_ref(case["rgb"], case["sem"], case["depth"], case["gt_rgb"],
                                    case["labels"], case["gt_depth"], case["uom"], W_SEM, W_DEPTH)
    want, wgrads = LN.torch_nerf(case, torch.float64, W_SEM, W_DEPTH)
    for k in range(7):
        _close(stats[k], want[k])
    assert stats[7] == 0.0
    assert np.isnan(stats[1]) == (kind == "all_invalid")
    assert np.isnan(stats[2]) == (kind == "no_depth")
    if case["zero_prob_row"] is not None and kind == "plain":
        assert case["zero_prob_row"] in case["huge_rows"]
        big = np.abs(grads[1][case["zero_prob_row"]]).max()
        assert np.isfinite(big) and big > 1e9 / N
    for g, w in zip(grads, wgrads):
        _rows_close(g, w, floor=1.0 / N)


def test_nerf_loss_ref_by_hand():
    # two rays, C = 2: row 0 = (0.25, 0.75) label 1; row 1 all zero (invalid)
    stats, (d_rgb, d_sem, d_depth) = LN.nerf_loss_ref(
        np.array([[0.5, 0.5, 0.5], [1.0, 0.0, 0.0]]), np.array([[0.25, 0.75], [0.0, 0.0]]),
        np.array([1.0, 2.0]), np.array([[0.0, 0.5, 0.5], [1.0, 0.0, 0.0]]), np.array([1, 0]),
        np.array([0.0, 3.0]), 0.5, 0.04, 0.1)
    assert stats[0] == 0.25 / 6 and stats[3] == 1 and stats[4] == 1
    assert abs(stats[1] - (-np.log(0.75 + 1e-15) / 2)) < 1e-15
    assert stats[2] == 1.0                               # |2 / 0.5 - 3|
    assert abs(stats[5] - (stats[0] + 0.04 * stats[1] + 0.1)) < 1e-15
    assert np.array_equal(d_depth, [0.0, 0.1 / 0.5])
    assert np.all(d_sem[1] == 0) and d_sem[0, 1] < 0 < d_sem[0, 0]
    assert abs(d_sem[0] @ np.array([0.25, 0.75])) < 1e-17    # scale-invariant in the row
    assert d_rgb[0, 0] == 2 * 0.5 / 6


def test_nerf_loss_ref_labels_outside_the_classes_are_ignored():
    """Deliberate difference from torch, which raises on a label >= C: the
    kernels' documented behaviour is to ignore it like -1."""
    case = LN.nerf_case(64, 3)
    a = LN.nerf_loss_ref(case["rgb"], case["sem"], case["depth"], case["gt_rgb"], case["labels"],
                         case["gt_depth"], 0.7, W_SEM, W_DEPTH)
    lab = LN.oracle_labels(case["labels"], 3)
    assert (lab != case["labels"]).sum() == 2
    b = LN.nerf_loss_ref(case["rgb"], case["sem"], case["depth"], case["gt_rgb"], lab,
                         case["gt_depth"], 0.7, W_SEM, W_DEPTH)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][1], b[1][1])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_nerf_loss_ref_reproduces_the_reference_fixture(tag):
    """G6 (the reference's own forward_nerf_train, fp32), to the precision the
    fp32 oracle is held to in tests/test_oracle_golden.py."""
    from tests.test_oracle_golden import _g6_case
    g = load_golden("g6_nerf_losses.npz")
    gt_rgb, labels, gt_depth = _g6_case(g, tag)
    stats, (d_rgb, d_sem, d_depth) = LN.nerf_loss_ref(
        g[f"{tag}_image"], g[f"{tag}_sem"], g[f"{tag}_depth"], gt_rgb, labels, gt_depth,
        float(g[f"{tag}_uom"]), W_SEM, W_DEPTH)
    assert bool(np.isnan(stats[1])) == bool(g[f"{tag}_sem_is_none"])
    assert abs(stats[0] - float(g[f"{tag}_loss_color"])) <= 1e-7
    assert abs(stats[2] - float(g[f"{tag}_loss_depth"])) <= 1e-6
    if not np.isnan(stats[1]):
        assert abs(stats[1] - float(g[f"{tag}_loss_sem"])) <= 1e-5
    assert abs(stats[5] - float(g[f"{tag}_total"])) <= 1e-6
    f = lambda k: g[k].double().numpy()
    assert np.abs(d_rgb - f(f"{tag}_g_image").reshape(-1, 3)).max() <= 1e-9
    assert np.abs(d_depth - f(f"{tag}_g_depth").reshape(-1)).max() <= 1e-9
    assert np.abs(d_sem - f(f"{tag}_g_sem").reshape(d_sem.shape)).max() <= 1e-7


def test_nerf_loss_apply_ref():
    rng = np.random.default_rng(0)
    grads = (rng.standard_normal((5, 3)), rng.standard_normal((5, 4)), rng.standard_normal(5))
    t = lambda x: torch.tensor(x, dtype=torch.float64)
    o = LN.nerf_loss_apply_ref(grads, t([2.0]), None, None, None, 0.04, 0.1)
    assert all(np.array_equal(a, 2.0 * b) for a, b in zip(o, grads))
    o = LN.nerf_loss_apply_ref(grads, None, None, t(0.04), None, 0.04, 0.1)
    assert np.all(o[0] == 0) and np.all(o[2] == 0) and np.array_equal(o[1], grads[1])
    o = LN.nerf_loss_apply_ref(grads, t(1.0), t(0.5), t(0.08), t(-0.1), 0.04, 0.1)
    _close(o[0], 1.5 * grads[0])
    _close(o[1], 3.0 * grads[1])
    assert np.all(o[2] == 0)
    # as autograd: the terms' own gradients are the stored ones over their weights
    x = torch.tensor(grads[1], dtype=torch.float64)
    _close(LN.nerf_loss_apply_ref(grads, 0.3, 0.2, 0.7, 1.1, 0.04, 0.1)[1],
           (x * 0.3 + (x / 0.04) * 0.7).numpy())


@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("C", [1, 2, 40, 64])
def test_semantic_postproc_ref_is_the_oracle_in_float64(N, C):
    s = LN.postproc_case(N, C)
    for scale in (1.0, 2.0 ** -100):
        x = s.astype(np.float64) * scale
        n, a = LN.semantic_postproc_ref(x)
        wn, wa = ol.semantic_postproc(torch.from_numpy(x))
        _close(n, wn.numpy())
        assert np.array_equal(a, wa.numpy())
        assert np.array_equal(a, LN.semantic_postproc_ref(s)[1])
    if N > 8:
        assert np.all(n[1] == 1.0 / C) and a[1] == 0


@pytest.mark.parametrize("shape,scale,kind", LN.SEG_CASES)
def test_seg_tail_ref_is_the_torch_modules_in_float64(shape, scale, kind):
    x, labels = LN.seg_case(shape, scale, kind)
    r = LN.seg_tail_ref(x, labels, grad_scale=64.0)
    w = LN.torch_seg(x, labels, torch.float64, grad_scale=64.0)
    _close(r["prob"], w["prob"])
    assert np.array_equal(r["argmax"], w["argmax"])
    assert abs(r["loss"] - w["loss"]) <= REL * max(abs(w["loss"]), 1e-300)
    _close(r["d_logits"], w["d_logits"], scale=max(float(np.abs(w["d_logits"]).max()), 1e-300))
    if kind == "all_ignored":
        assert r["loss"] == 0.0 and not r["d_logits"].any()
    if kind == "ties":
        top2 = np.sort(x, axis=1)[:, -2:]
        assert (top2[:, 0] == top2[:, 1]).mean() >= 0.3
    no_labels = LN.seg_tail_ref(x)
    assert no_labels["loss"] is None and np.array_equal(no_labels["prob"], r["prob"])


def test_confusion_ref_reproduces_the_meter_golden():
    g = load_golden("g7_meter.npz")
    C = g["C"]
    cm = LN.confusion_ref(g["preds"], g["truths"], C)
    assert cm.dtype == np.int64 and np.array_equal(cm, g["conf_mat"].numpy())
    half = LN.confusion_ref(g["preds"][:2], g["truths"][:2], C)
    assert np.array_equal(LN.confusion_ref(g["preds"][2:], g["truths"][2:], C, cm0=half), cm)
    p, t = LN.confusion_case(255, 41)
    for bad in (-1, 41, 255, 2 ** 40, -2 ** 40):
        assert (p == bad).any() and (t == bad).any()
    cm = LN.confusion_ref(p, t, 41)
    assert cm.sum() == ((p >= 0) & (p < 41) & (t >= 0) & (t < 41)).sum() < 255
    assert cm[t[0], p[0]] >= 1


@pytest.mark.parametrize("wd", [0.0, 1e-6])
def test_adam_ref_is_the_oracle_and_torch_adam_in_float64(wd):
    rng = np.random.default_rng(3)
    n = 1025
    p0 = rng.standard_normal(n)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    tp = torch.tensor(p0, dtype=torch.float64).requires_grad_()
    opt = torch.optim.Adam([tp], lr=1e-2, betas=(0.9, 0.99), eps=1e-15, weight_decay=wd)
    op, om, ov = (torch.tensor(a) for a in (p, m, v))
    for step in (1, 2, 3):
        g = LN.adam_grads(rng, n).astype(np.float64)
        p, m, v = LN.adam_ref(p, g * 8.0, m, v, step, 1e-2, 0.9, 0.99, 1e-15, wd, 1.0 / 8.0)
        op, om, ov = ol.adam_step(op, torch.tensor(g), om, ov, step, 1e-2, weight_decay=wd)
        tp.grad = torch.tensor(g)
        opt.step()
        for a, b in ((p, op), (m, om), (v, ov), (p, tp.detach()),
                     (m, opt.state[tp]["exp_avg"]), (v, opt.state[tp]["exp_avg_sq"])):
            _close(a, b.numpy())


def test_adam_scaled_ref_skips_without_counting():
    rng = np.random.default_rng(4)
    n = 257
    p0 = rng.standard_normal(n)
    grads = [LN.adam_grads(rng, n).astype(np.float64) for _ in range(4)]
    kw = dict(lr=1e-2, b1=0.9, b2=0.99, eps=1e-15, wd=1e-6)
    hist, skipped = LN.adam_scaled_ref(p0, [g * 1024.0 for g in grads], np.zeros(n), np.zeros(n),
                                       [0, 1, 0, 0], [1024.0] * 4, **kw)
    assert skipped == 1 and len(hist) == 4
    assert all(np.array_equal(a, b) for a, b in zip(hist[0], hist[1]))   # step 2 untouched
    # = three plain steps numbered 1, 2, 3 on the gradients of steps 1, 3, 4
    p, m, v = p0, np.zeros(n), np.zeros(n)
    for step, g in zip((1, 2, 3), (grads[0], grads[2], grads[3])):
        p, m, v = LN.adam_ref(p, g, m, v, step, 1e-2, 0.9, 0.99, 1e-15, 1e-6)
    for a, b in zip(hist[3], (p, m, v)):
        _close(a, b)
