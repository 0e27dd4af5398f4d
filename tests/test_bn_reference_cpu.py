"""tests/bn_numpy.py is right and its bounds bite.  No GPU.

* The float64 restatement equals ``nn.BatchNorm2d`` in double (+ add + relu,
  autograd) to 1e-12 of each output's largest magnitude (of the absolute terms
  for the two sums dgamma and dbeta), on every case with
  M >= 2, and over three steps of ``momentum=None``, with ``affine=False`` and
  with ``track_running_stats=False``.
* Two fp32 evaluations stay inside the derived bounds (err / bound <= 1 for
  every element of every output): the emulation of the kernels' own summation
  order and coefficient arithmetic, and torch's CPU fp32 ``F.batch_norm`` + add
  + relu / ``native_batch_norm_backward``.  The worst ratios are printed at the
  end (docs/DESIGN_NOTEBOOK.md keeps the table).
* Each deliberate mistake of ``bn_numpy.MUTANTS``, made in the fp32 emulation,
  is rejected by the ``compare_*`` call of the named case in ``REJECTED_BY``.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import bn_numpy as bn

F64 = np.float64
SMALL = [n for n in bn.SHAPE_NAMES if not n.startswith("stride")]
ALL = SMALL + list(bn.EVAL_NAMES) + list(bn.OFFSET_NAMES) + list(bn.SYNTH_NAMES)
STRIDE = bn.SHAPE_NAMES[-1]


def _cases(names):
    out = []
    for n in names:
        out.append((n, "f32"))
        if n not in bn.OFFSET_NAMES:
            out.append((n, "bf16"))
    return out


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    return bn.build_case(name, dtype)


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    if bn.WORST:
        print("\nworst err / bound per evaluation, type, case family and output:")
        for k in sorted(bn.WORST):
            print(f"  {k}: {bn.WORST[k]:.3f}")


def _t(a, dt=torch.float64):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _rel(got, ref, what, scale=None):
    """1e-12 of the output's largest magnitude (of a sum's absolute terms where
    ``scale`` gives them: dy orthogonal to xhat makes dgamma cancel to ~0)"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    err = float(np.abs(got - ref).max())
    scale = float(np.abs(ref).max()) if scale is None else float(np.max(scale))
    assert err <= 1e-12 * max(scale, 1e-300), (what, err)


# ---------------------------------------------------------------------------
# the restatement of bn_geom
# ---------------------------------------------------------------------------
def test_geometry_reaches_the_paths_the_cases_are_named_for():
    g = bn.geom(70, 64)
    assert (g.tq, g.rows_per_it, g.rows_per_wg) == (16, 16, 64)
    assert [bn.geom(70, C).tq for C in (4, 12, 16, 32)] == [1, 1, 4, 8]
    assert [bn.geom(70, C).n_col_wg for C in (12, 24, 72, 136, 4096)] == [3, 3, 9, 17, 64]
    assert bn.geom(255, 4).rows_per_it == 256
    # a last workgroup holding a single row
    for M, C in ((65, 64), (129, 64), (1025, 4)):
        g = bn.geom(M, C)
        assert M - (g.n_row_wg - 1) * g.rows_per_wg == 1 and g.n_row_wg >= 2
    # n_row_wg at its cap: bn_group_reduce's unrolled loop runs (16 row lanes)
    assert [bn.geom(M, 64).n_row_wg for M in bn.CAP_M] == [128, 128, 103]
    assert 3 * bn.geom(8192, 64).rows_per_it < 128
    N, C, H, W = bn.STRIDE_SHAPE
    assert N * H * W * (C // 4) > bn.APPLY_QUADS
    assert (N * H * W - 1) * (C // 4) >= bn.APPLY_QUADS      # ... by more than a partial row


@pytest.mark.parametrize("name,dtype", _cases(ALL), ids=lambda v: v)
def test_every_relu_decision_is_pinned(name, dtype):
    c = _case(name, dtype)
    if c.relu:
        r = c.ref
        assert ((np.abs(r.pre) >= 4.0 * r.e_pre) | (r.e_pre == 0)).all()


# ---------------------------------------------------------------------------
# against torch in double
# ---------------------------------------------------------------------------
def _torch64(c, training=True):
    """nn.BatchNorm2d in double on the case (+ add + relu), autograd with dy."""
    m = nn.BatchNorm2d(c.C, eps=float(np.float32(c.eps)), momentum=float(np.float32(c.momentum)),
                       affine=c.gamma is not None, track_running_stats=c.running_mean is not None).double()
    with torch.no_grad():
        if c.gamma is not None:
            m.weight.copy_(_t(c.gamma))
            m.bias.copy_(_t(c.beta))
        if c.running_mean is not None:
            m.running_mean.copy_(_t(c.running_mean))
            m.running_var.copy_(_t(c.running_var))
    m.train(training)
    x = _t(c.x).reshape(c.M, c.C, 1, 1).requires_grad_()
    res = None if c.res is None else _t(c.res).reshape(c.M, c.C, 1, 1).requires_grad_()
    y = m(x)
    if res is not None:
        y = y + res
    if c.relu:
        y = F.relu(y)
    y.backward(_t(c.dy).reshape(c.M, c.C, 1, 1))
    return m, x, res, y


@pytest.mark.parametrize("name,dtype", [(n, d) for n, d in _cases(ALL) + [(STRIDE, "f32")]
                                        if "-M1[" not in n + "["], ids=lambda v: v)
def test_restatement_equals_torch_in_double(name, dtype):
    c = _case(name, dtype)
    m, x, res, y = _torch64(c, c.training)
    r = c.ref
    flat = lambda t: t.detach().reshape(c.M, c.C).numpy()
    _rel(r.y, flat(y), "y")
    if c.training and c.running_mean is not None:
        _rel(r.new_running_mean, m.running_mean.numpy(), "running_mean")
        _rel(r.new_running_var, m.running_var.numpy(), "running_var")
    if not c.training:
        return
    # the backward on the forward's own y and float64 statistics is autograd's
    b = bn.backward(c.dy, c.x, r.y, c.gamma, r.mean, r.invstd, c.relu)
    _rel(b.dx, flat(x.grad), "dx")
    if res is not None:
        _rel(b.dres, flat(res.grad), "dres")
    if c.gamma is not None:
        xh = (c.x.astype(F64) - r.mean) * r.invstd
        _rel(b.dgamma, m.weight.grad.numpy(), "dgamma", np.abs(b.dres * xh).sum(0))
        _rel(b.dbeta, m.bias.grad.numpy(), "dbeta", np.abs(b.dres).sum(0))
    _rel(r.save_mean, flat(x).mean(0), "save_mean")


@pytest.mark.parametrize("kw", [dict(momentum=None), dict(affine=False), dict(track_running_stats=False)],
                         ids=["momentum-none", "affine-false", "no-running-stats"])
def test_module_variants_over_three_steps_in_double(kw):
    rng = np.random.default_rng(7)
    M, C = 37, 8
    m = nn.BatchNorm2d(C, **kw).double().train()
    rm = None if m.running_mean is None else m.running_mean.numpy().copy()
    rv = None if m.running_var is None else m.running_var.numpy().copy()
    for step in range(1, 4):
        x = rng.standard_normal((M, C)) * 1.3 + 0.4
        y = m(_t(x).reshape(M, C, 1, 1))
        mom = 1.0 / step if "momentum" in kw else 0.1
        gam = None if m.weight is None else m.weight.detach().numpy()
        bet = None if m.bias is None else m.bias.detach().numpy()
        r = bn.forward(x, None, gam, bet, rm, rv, mom, m.eps, False, True, round_args=False)
        _rel(r.y, y.detach().reshape(M, C).numpy(), "y")
        if rm is not None:
            rm, rv = r.new_running_mean, r.new_running_var
            _rel(rm, m.running_mean.numpy(), "running_mean")
            _rel(rv, m.running_var.numpy(), "running_var")
            assert int(m.num_batches_tracked) == step
    # eval mode of the same module normalises with what has accumulated
    if rm is not None:
        m.eval()
        y = m(_t(x).reshape(M, C, 1, 1))
        r = bn.forward(x, None, gam, bet, rm, rv, 0.1, m.eps, False, False, round_args=False)
        _rel(r.y, y.detach().reshape(M, C).numpy(), "eval y")


# ---------------------------------------------------------------------------
# fp32 evaluations stay inside the bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", _cases(ALL) + [(STRIDE, "f32")], ids=lambda v: v)
def test_kernel_order_emulation_is_inside_the_bounds(name, dtype):
    c = _case(name, dtype)
    e = bn.emulate_forward(*bn.forward_args(c), dtype=dtype)
    bn.compare_forward(e, c.ref, f"emulation fwd {dtype} {c.family}", c.name)
    eb = bn.emulate_backward(*bn.backward_args(c), dtype=dtype)
    bn.compare_backward(eb, bn.ref_backward(c), f"emulation bwd {dtype} {c.family}", c.name)


@pytest.mark.parametrize("name", ALL, ids=lambda v: v)
def test_torch_cpu_fp32_is_inside_the_bounds(name):
    """F.batch_norm + add + relu in fp32 on the CPU; the backward through
    ``native_batch_norm_backward`` so that it receives the case's pinned mean /
    invstd as the kernel does (autograd would use torch's own statistics).

    torch does not share the kernels' geometry: it sums a channel's M terms in
    fp32 without a shift and far deeper than ``depth`` (9600 equal values come
    back 60 ulp off), and updates the running statistics in fp32.  It is held
    to the SAME formulas with those three counts replaced (``model="generic"``:
    shift 0, depth M, three more roundings in the update).  Under the kernel's
    own counts it exceeds the bounds exactly there: running_var 1.03 at M = 2,
    running_mean 1.13 at mean 1000, y of a constant channel 3.3, and the
    settled-shift cases, whose accuracy torch does not have."""
    c = _case(name, "f32")
    ref = bn.ref_forward(c, "generic")
    f32 = torch.float32
    x = _t(c.x, f32).reshape(c.M, c.C, 1, 1)
    rm, rv = _t(c.running_mean, f32), _t(c.running_var, f32)
    eps = float(np.float32(c.eps))
    # torch.batch_norm: F.batch_norm refuses M = 1 in training mode
    y = torch.batch_norm(x, _t(c.gamma, f32), _t(c.beta, f32), rm, rv, c.training,
                         float(np.float32(c.momentum)), eps, False)
    if c.res is not None:
        y = y + _t(c.res, f32).reshape(c.M, c.C, 1, 1)
    if c.relu:
        y = F.relu(y)
    got = dict(y=y.reshape(c.M, c.C).numpy())
    if c.training and rm is not None:
        got.update(new_running_mean=rm.numpy(), new_running_var=rv.numpy())
    # M = 1: torch's unbiased variance is 0 / 0; the kernel's rule (factor 1) is its own
    names = [k for k in ("y", "new_running_mean", "new_running_var")
             if k in got and not (k == "new_running_var" and c.M == 1)]
    bn.compare_outputs(names, got, ref, f"torch-fp32 fwd {c.family}", c.name, True)
    if not c.training:
        return
    rb = bn.ref_backward(c, "generic")
    g = _t(rb.dres, f32).reshape(c.M, c.C, 1, 1)          # dy * (y > 0): exact
    dx, dw, db = torch.ops.aten.native_batch_norm_backward(
        g, x, _t(c.gamma, f32), None, None, _t(c.bmean, f32), _t(c.binvstd, f32), True, eps,
        [True, True, True])
    got = dict(dx=dx.reshape(c.M, c.C).numpy(), dgamma=dw.numpy(), dbeta=db.numpy())
    bn.compare_backward(got, rb, f"torch-fp32 bwd {c.family}", c.name, names=("dx", "dgamma", "dbeta"))


def test_settled_statistics_are_as_tight_as_no_offset():
    """The header's claim: with running_mean at the batch mean the variance
    does not cancel -- the derived bound of invstd at ratio 10, 100 and 1000 is
    that of ratio 0, while with shift 0 it grows with the square of the ratio."""
    rel = {}
    for name in bn.OFFSET_NAMES:
        r = _case(name, "f32").ref
        rel[name] = r.e_save_invstd / r.save_invstd
        print(name, "relative bound of invstd per channel:", " ".join(f"{v:.2e}" for v in rel[name]))
    s, z = rel["offset-settled"], rel["offset-rm0"]
    assert (s[1:6] <= 1.5 * s[0]).all() and s[0] <= 2e-6
    assert z[1] > 10 * z[0] and z[2] > 50 * z[1] and z[3] > 50 * z[2]
    assert np.allclose(z, rel["offset-null"], rtol=0.05)      # NULL statistics: the same shift 0


# ---------------------------------------------------------------------------
# the bounds bite: every mutant is rejected by a named case
# ---------------------------------------------------------------------------
REJECTED_BY = {
    "biased_running_var": ("fwd", "column-C4", "f32"),
    "unbiased_normalises": ("fwd", "column-C4", "f32"),
    "momentum_swapped": ("fwd", "column-C4", "f32"),
    "eps_outside_sqrt": ("fwd", "offset-settled", "f32"),
    "shift_not_added": ("fwd", "column-C4", "f32"),
    "running_mean_shifted": ("fwd", "column-C4", "f32"),
    "res_after_relu": ("fwd", "column-C4", "f32"),
    "mask_from_x": ("bwd", "column-C4", "f32"),
    "mask_ge": ("bwd", "column-C4", "f32"),
    "dres_unmasked": ("bwd", "column-C4", "f32"),
    "dgamma_from_x": ("bwd", "column-C4", "f32"),
    "dx_no_mean_g": ("bwd", "column-C4", "f32"),
    "dx_no_xhat": ("bwd", "column-C4", "f32"),
    "dx_m_minus_1": ("bwd", "column-C4", "f32"),
    "tail_rows_dropped": ("both", "row-C64-M17", "f32"),
    "last_wg_dropped": ("both", "row-C64-M65", "f32"),
    "quads_swapped": ("both", "column-C8", "f32"),
    "second_pass_skipped": ("both", STRIDE, "f32"),
    "bf16_truncated": ("both", "column-C4", "bf16"),
    "nan_zeroed": ("nan", "column-C8", "f32"),
}


def test_the_mutant_table_is_complete():
    assert set(REJECTED_BY) == set(bn.MUTANTS) and len(bn.MUTANTS) == 20


@pytest.mark.parametrize("mutant", bn.MUTANTS)
def test_mutant_is_rejected(mutant):
    how, name, dtype = REJECTED_BY[mutant]
    c = _case(name, dtype)
    mu = (mutant,)
    if how == "nan":
        d = bn.with_nan(c, 3, 5)
        assert d.relu
        good = bn.emulate_forward(*bn.forward_args(d), dtype=dtype)
        bn.compare_nan_forward(good.y, good.save_mean, d, c.ref)
        bad = bn.emulate_forward(*bn.forward_args(d), dtype=dtype, mutant=mu)
        with pytest.raises(bn.Mismatch):
            bn.compare_nan_forward(bad.y, bad.save_mean, d, c.ref)
        return
    if how in ("fwd", "both"):
        e = bn.emulate_forward(*bn.forward_args(c), dtype=dtype, mutant=mu)
        with pytest.raises(bn.Mismatch):
            bn.compare_forward(e, c.ref, "mutant", c.name, record=False)
    if how in ("bwd", "both"):
        e = bn.emulate_backward(*bn.backward_args(c), dtype=dtype, mutant=mu)
        with pytest.raises(bn.Mismatch):
            bn.compare_backward(e, bn.ref_backward(c), "mutant", c.name, record=False)


def test_subnormal_y_passes_the_gradient_and_minus_zero_does_not():
    for dtype in ("f32", "bf16"):
        c = _case("column-C8", dtype)
        assert c.relu
        sub = c.y == np.float32(bn.SUB[dtype])
        neg0 = (c.y == 0) & np.signbit(c.y)
        assert sub.sum() >= 4 and neg0.sum() >= 4 and ((c.y == 0) & ~np.signbit(c.y)).any()
        rb = bn.ref_backward(c)
        assert np.array_equal(rb.dres[sub], c.dy.astype(F64)[sub]) and (rb.dres[neg0] == 0).all()
        t = torch.from_numpy(c.y).requires_grad_()
        torch.relu(t).backward(torch.from_numpy(c.dy))
        assert np.array_equal(t.grad.numpy().astype(F64)[sub], rb.dres[sub])
