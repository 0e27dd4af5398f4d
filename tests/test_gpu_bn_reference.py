"""``ops.bn_act_fwd`` / ``ops.bn_act_bwd`` (csrc/batchnorm.hip, six kernels)
against the float64 restatement of tests/bn_numpy.py, element by element, within
the bounds derived there from counting rounding steps: one test id = one entry
point on one case, fp32 and bf16, every output.  The case builders pin every
ReLU decision, so there are no exempt elements.  The backward is called on its
own, with synthetic ``y`` (zeros, -0.0, subnormals) and ``mean`` / ``invstd``
that are not the statistics of ``x``.  tests/test_bn_reference_cpu.py holds the
restatement against torch in double and shows that the same ``compare_*`` calls
reject twenty deliberate mistakes.

Worst err / bound per entry point and case family, as printed at the end of a
run on an MI355X: docs/DESIGN_NOTEBOOK.md, "Float64 per-element parity of the
fused BatchNorm kernels"."""
import functools

import numpy as np
import pytest
import torch

from tests import bn_numpy as bn

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
BOTH = ("f32", "bf16")


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    yield _ops
    if bn.WORST:
        print("\nworst err / bound per entry point, type, case family and output:")
        for k in sorted(bn.WORST):
            print(f"  {k}: {bn.WORST[k]:.3f}")


@functools.lru_cache(maxsize=None)
def _case(name, dtype):
    return bn.build_case(name, dtype)


def _vec(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


def _act(a, c):
    """[M, C] values -> the channels_last [N, C, H, W] tensor of the case's type"""
    if a is None:
        return None
    N, C, H, W = c.shape
    t = torch.from_numpy(np.ascontiguousarray(a, F32)).cuda().to(TD[c.dtype])
    return t.reshape(N, H, W, C).permute(0, 3, 1, 2)


def _rows(t):
    if t is None:
        return None
    if t.dim() == 1:
        return t.double().cpu().numpy()
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu().numpy()


def _fwd(ops, c, x=None, relu=None, training=None):
    rm, rv = _vec(c.running_mean), _vec(c.running_var)
    y, mean, invstd = ops.bn_act_fwd(_act(c.x if x is None else x, c), _act(c.res, c), _vec(c.gamma),
                                     _vec(c.beta), rm, rv, c.momentum, c.eps,
                                     c.relu if relu is None else relu,
                                     c.training if training is None else training)
    torch.cuda.synchronize()
    upd = (c.training if training is None else training) and rm is not None
    return dict(y=y, save_mean=mean, save_invstd=invstd, new_running_mean=rm if upd else None,
                new_running_var=rv if upd else None, rm=rm, rv=rv)


def _np_out(out, names):
    return {k: _rows(out[k]) for k in names}


def _bwd(ops, c, want_dres=None, want_dwb=None, y=None, mean=None, invstd=None):
    want_dres = c.want_dres if want_dres is None else want_dres
    want_dwb = c.want_dwb if want_dwb is None else want_dwb
    yy = (_act(c.y, c) if y is None else y) if c.relu else None
    dx, dres, dw, db = ops.bn_act_bwd(_act(c.dy, c), _act(c.x, c), yy, _vec(c.gamma),
                                      _vec(c.bmean) if mean is None else mean,
                                      _vec(c.binvstd) if invstd is None else invstd,
                                      c.relu, want_dres, want_dwb)
    torch.cuda.synchronize()
    return dict(dx=dx, dres=dres, dgamma=dw, dbeta=db)


def _ids(names, dtypes=BOTH):
    return [pytest.param(n, d, id=f"{n}-{d}") for n in names for d in dtypes]


# ---------------------------------------------------------------------------
# every output of every case within its bound
# ---------------------------------------------------------------------------
FWD_CASES = _ids(bn.SHAPE_NAMES) + _ids(bn.OFFSET_NAMES, ("f32",)) + _ids(bn.SYNTH_NAMES)
BWD_CASES = _ids(bn.SHAPE_NAMES) + _ids(bn.OFFSET_NAMES, ("f32",)) + _ids(bn.SYNTH_NAMES)


@pytest.mark.parametrize("name,dtype", FWD_CASES)
def test_forward(ops, name, dtype):
    """training mode: y, save_mean, save_invstd and the running statistics.
    The offset cases hold save_invstd and y to the derived bounds at ratios
    |mean - shift| / std up to 1000 with shift 0, and to the bound of ratio 0
    with a settled running_mean."""
    c = _case(name, dtype)
    out = _fwd(ops, c)
    assert out["y"].dtype == TD[dtype] and out["y"].is_contiguous(memory_format=torch.channels_last)
    bn.compare_forward(_np_out(out, bn.FWD_OUT), c.ref, f"fwd {dtype} {c.family}", c.name)
    if c.running_mean is not None and c.momentum == 0.0:
        assert torch.equal(out["rm"], _vec(c.running_mean)) and torch.equal(out["rv"], _vec(c.running_var))


@pytest.mark.parametrize("name,dtype", BWD_CASES)
def test_backward(ops, name, dtype):
    """dx, dresidual, dgamma, dbeta on pinned inputs; outputs that are not
    requested come back as None."""
    c = _case(name, dtype)
    out = _bwd(ops, c)
    names = ["dx"] + (["dres"] if c.want_dres else []) + (["dgamma", "dbeta"] if c.want_dwb else [])
    for k in bn.BWD_OUT:
        assert (out[k] is None) == (k not in names), k
    bn.compare_backward(_np_out(out, names), bn.ref_backward(c), f"bwd {dtype} {c.family}", c.name, names=names)


@pytest.mark.parametrize("name,dtype", _ids(bn.EVAL_NAMES))
def test_eval_forward(ops, name, dtype):
    """the running statistics normalise: y within its bound, the buffers
    byte-identical, save_* None"""
    c = _case(name, dtype)
    out = _fwd(ops, c)
    assert out["save_mean"] is None and out["save_invstd"] is None
    assert torch.equal(out["rm"], _vec(c.running_mean)) and torch.equal(out["rv"], _vec(c.running_var))
    bn.compare(_rows(out["y"]), c.ref.y, c.ref.e_y, f"fwd-eval {dtype} eval y @ {c.name}")


# ---------------------------------------------------------------------------
# bit-exact properties
# ---------------------------------------------------------------------------
def _bytes_equal(a, b):
    bits = lambda t: t.view(torch.int32 if t.element_size() == 4 else torch.int16)
    return all((u is None and v is None) or torch.equal(bits(u), bits(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype", BOTH)
def test_repeated_and_interleaved_calls_give_equal_bytes(ops, dtype):
    """A repeated call gives equal bytes; so does the same case after a larger
    one has used (and grown) the same scratch buffer."""
    c, big = _case("row-C64-M129", dtype), _case("column-C4096", dtype)
    keys_f, keys_b = ("y", "save_mean", "save_invstd", "rm", "rv"), bn.BWD_OUT
    f0, b0 = _fwd(ops, c), _bwd(ops, c)
    f1, b1 = _fwd(ops, c), _bwd(ops, c)
    _fwd(ops, big), _bwd(ops, big)
    f2, b2 = _fwd(ops, c), _bwd(ops, c)
    for f, b in ((f1, b1), (f2, b2)):
        assert _bytes_equal([f0[k] for k in keys_f], [f[k] for k in keys_f])
        assert _bytes_equal([b0[k] for k in keys_b], [b[k] for k in keys_b])


@pytest.mark.parametrize("dtype", BOTH)
def test_dx_does_not_depend_on_dresidual_being_requested(ops, dtype):
    c = _case("column-C72", dtype)
    a, b = _bwd(ops, c, want_dres=True, want_dwb=True), _bwd(ops, c, want_dres=False, want_dwb=False)
    assert b["dres"] is None and b["dgamma"] is None and b["dbeta"] is None
    assert _bytes_equal([a["dx"]], [b["dx"]])


@pytest.mark.parametrize("dtype", BOTH)
def test_nothing_is_written_beyond_the_outputs(ops, dtype):
    """The raw entry points with guard bytes after y, dx, dresidual, the
    per-channel outputs and the workspace: all intact; eval mode leaves save_*
    and the running statistics alone."""
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd.ops._args import _ptr, _stream
    c = _case("column-C64", dtype)             # 1120 quads: the last block of the apply grid is partial
    assert c.relu and c.res is not None and c.running_mean is not None
    M, C, n, G = c.M, c.C, c.M * c.C, 256
    td, code = TD[dtype], 0 if dtype == "f32" else 1
    flat = lambda a: torch.from_numpy(np.ascontiguousarray(a, F32)).cuda().to(td).reshape(-1)
    guard = lambda k, dt=td: torch.full((k + G,), -77.0, device="cuda", dtype=dt)
    nws = int(_lib.lib().ucsa_bn_workspace_bytes(M, C))
    ws = torch.full((nws + G,), 0x5A, device="cuda", dtype=torch.uint8)
    x, res, dy, yin = flat(c.x), flat(c.res), flat(c.dy), flat(c.y)
    # named, so that they outlive the calls that only receive their addresses
    gam, bet, bmean, binvstd = _vec(c.gamma), _vec(c.beta), _vec(c.bmean), _vec(c.binvstd)
    for training in (1, 0):
        y, sm, si = guard(n), guard(C, torch.float32), guard(C, torch.float32)
        rm, rv = _vec(c.running_mean), _vec(c.running_var)
        _lib.check(_lib.lib().ucsa_bn_act_fwd(
            _ptr(x), _ptr(res), _ptr(gam), _ptr(bet), _ptr(rm), _ptr(rv),
            float(c.momentum), float(c.eps), M, C, int(c.relu), training, code, _ptr(y), _ptr(sm),
            _ptr(si), _ptr(ws), _stream()), "ucsa_bn_act_fwd")
        torch.cuda.synchronize()
        assert (y[n:] == -77.0).all() and (sm[C:] == -77.0).all() and (si[C:] == -77.0).all()
        assert (ws[nws:] == 0x5A).all()
        want = bn.forward(*bn.forward_args(c)[:-1], bool(training), dtype=dtype)
        bn.compare(y[:n].double().cpu().numpy().reshape(M, C), want.y, want.e_y,
                   f"raw {dtype} guard y @ {c.name}", record=False)
        if not training:
            assert (sm == -77.0).all() and (si == -77.0).all()
            assert torch.equal(rm, _vec(c.running_mean)) and torch.equal(rv, _vec(c.running_var))
    for want_dres in (True, False):
        dx, dres = guard(n), guard(n)
        dw, db = guard(C, torch.float32), guard(C, torch.float32)
        _lib.check(_lib.lib().ucsa_bn_act_bwd(
            _ptr(dy), _ptr(x), _ptr(yin), _ptr(gam), _ptr(bmean), _ptr(binvstd),
            M, C, int(c.relu), code, _ptr(dx), _ptr(dres) if want_dres else None,
            _ptr(dw) if want_dres else None, _ptr(db) if want_dres else None, _ptr(ws), _stream()),
            "ucsa_bn_act_bwd")
        torch.cuda.synchronize()
        assert (dx[n:] == -77.0).all() and (ws[nws:] == 0x5A).all()
        assert (dres[n:] == -77.0).all() and (dw[C:] == -77.0).all() and (db[C:] == -77.0).all()
        if not want_dres:                       # not requested: not written
            assert (dres == -77.0).all() and (dw == -77.0).all() and (db == -77.0).all()
        rb = bn.ref_backward(c)
        bn.compare(dx[:n].double().cpu().numpy().reshape(M, C), rb.dx, rb.e_dx,
                   f"raw {dtype} guard dx @ {c.name}", record=False)


# ---------------------------------------------------------------------------
# non-finite input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("dtype", BOTH)
def test_nan_in_training_poisons_its_channel_only(ops, dtype, relu):
    """One NaN in x: every y of that channel is NaN with and without the ReLU
    (F.batch_norm + relu propagates it; v > 0 ? v : 0 gave zeros), save_mean is
    NaN, dx of the channel is non-finite; the other channels are untouched."""
    c = _case("column-C8", dtype)
    assert c.relu and c.res is None
    d = bn.with_nan(c, 3, 5)
    ref = c.ref if relu else bn.forward(*bn.forward_args(c)[:-2], False, True, dtype=dtype)
    out = _fwd(ops, d, relu=relu)
    bn.compare_nan_forward(_rows(out["y"]), _rows(out["save_mean"]), d, ref)
    d.relu = relu
    dx = _rows(_bwd(ops, d, y=out["y"], mean=out["save_mean"], invstd=out["save_invstd"])["dx"])
    assert not np.isfinite(dx[:, 5]).any()
    assert np.isfinite(np.delete(dx, 5, axis=1)).all()


@pytest.mark.parametrize("dtype", BOTH)
def test_nonfinite_in_eval_mode_stays_in_its_element(ops, dtype):
    c = _case("eval-C72-M70", dtype)
    assert c.relu and not c.training
    ch = int(np.argmax(c.gamma > 0))
    for value in (np.nan, np.inf):
        d = bn.with_nan(c, 7, ch, value)
        y = _rows(_fwd(ops, d)["y"])
        assert np.isnan(y[7, ch]) if np.isnan(value) else y[7, ch] == np.inf
        y[7, ch] = c.ref.y[7, ch]
        bn.compare(y, c.ref.y, c.ref.e_y, f"eval nonfinite @ {c.name}", record=False)


# ---------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------
def _module_steps(monkeypatch, ops, kw, dtype, steps=3):
    """``FusedBatchNorm2d(**kw)`` over ``steps`` training steps on fresh
    batches; every step's y, buffers, num_batches_tracked and gradients against
    the restatement fed with the buffers the module held before the step and
    (for the backward) the save_mean / save_invstd the forward op returned."""
    from ucsa_neural_rendering_amd.network.fused_bn import FusedBatchNorm2d, _fusable
    seen = []
    real = ops.bn_act_fwd
    monkeypatch.setattr(ops, "bn_act_fwd", lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1])
    rng = np.random.default_rng(11)
    shape, M, C = (2, 8, 5, 7), 70, 8
    m = FusedBatchNorm2d(C, **kw).cuda().train()
    c = bn.NS(shape=shape, dtype=dtype)
    fam = "module"
    for step in range(1, steps + 1):
        x = bn.to_dtype(rng.standard_normal((M, C)) * 1.3 + 0.4, dtype)
        dy = bn.to_dtype(rng.standard_normal((M, C)), dtype)
        before = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
        xg = _act(x, c).detach().requires_grad_()
        assert _fusable(xg)
        y = m(xg)
        assert len(seen) == step
        y.backward(_act(dy, c))
        torch.cuda.synchronize()
        mom = (1.0 / step if m.momentum is None else m.momentum) if m.track_running_stats else 0.0
        gam, bet = before.get("weight"), before.get("bias")
        r = bn.forward(x, None, gam, bet, before.get("running_mean"), before.get("running_var"), mom,
                       m.eps, False, True, dtype=dtype)
        got = dict(y=_rows(y.detach()), save_mean=_rows(seen[-1][1]), save_invstd=_rows(seen[-1][2]),
                   new_running_mean=_rows(m.running_mean), new_running_var=_rows(m.running_var))
        bn.compare_forward(got, r, f"module-fwd {dtype} {fam}", f"{kw} step {step}")
        if m.track_running_stats:
            assert int(m.num_batches_tracked) == step
        rb = bn.backward(dy, x, None, gam, got["save_mean"], got["save_invstd"], False, dtype=dtype)
        names = ["dx"] + (["dgamma", "dbeta"] if m.affine else [])
        gb = dict(dx=_rows(xg.grad), dgamma=_rows(m.weight.grad) if m.affine else None,
                  dbeta=_rows(m.bias.grad) if m.affine else None)
        bn.compare_backward(gb, rb, f"module-bwd {dtype} {fam}", f"{kw} step {step}", names=names)
        if m.affine:
            m.weight.grad = m.bias.grad = None
            with torch.no_grad():                   # parameters that are not 1 and 0 next step
                m.weight.add_(0.25 * step)
                m.bias.sub_(0.125 * step)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("kw", [dict(momentum=None), dict(affine=False), dict(track_running_stats=False)],
                         ids=["momentum-none", "affine-false", "no-running-stats"])
def test_module_variants(monkeypatch, ops, kw, dtype):
    _module_steps(monkeypatch, ops, kw, dtype)


@pytest.mark.parametrize("dtype", BOTH)
def test_module_eval_backward(ops, dtype):
    """The eval-mode backward of ``_BnActFn`` is plain torch: dx = g * k with
    k = gamma * rsqrt(running_var + eps) rounded to the activation's type BEFORE
    the product (``bn_numpy.eval_backward`` says so in its bound), dresidual = g
    exactly, dgamma / dbeta fp32 sums."""
    from ucsa_neural_rendering_amd.network.fused_bn import FusedBatchNorm2d, _fusable
    c = _case("eval-C72-M70", dtype)
    m = FusedBatchNorm2d(c.C, eps=c.eps).cuda().eval()
    with torch.no_grad():
        m.weight.copy_(_vec(c.gamma))
        m.bias.copy_(_vec(c.beta))
        m.running_mean.copy_(_vec(c.running_mean))
        m.running_var.copy_(_vec(c.running_var))
    xg, rg = _act(c.x, c).detach().requires_grad_(), _act(c.res, c).detach().requires_grad_()
    assert _fusable(xg)
    y = m(xg, residual=rg, relu=True)
    y.backward(_act(c.dy, c))
    torch.cuda.synchronize()
    yv = _rows(y.detach())
    bn.compare(yv, c.ref.y, c.ref.e_y, f"module-eval {dtype} eval y @ {c.name}")
    rb = bn.eval_backward(c.dy, c.x, yv, c.gamma, c.running_mean, c.running_var, c.eps, True, dtype=dtype)
    got = dict(dx=_rows(xg.grad), dres=_rows(rg.grad), dgamma=_rows(m.weight.grad), dbeta=_rows(m.bias.grad))
    bn.compare_backward(got, rb, f"module-eval-bwd {dtype} eval", c.name)
