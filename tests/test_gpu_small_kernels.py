"""The kernels that close the training loop (csrc/losses.hip, csrc/optim.hip)
against the float64 yardstick tests/losses_numpy.py at the shapes where such
kernels go wrong: one element, partial tail blocks, a wave across two batch
images, C = 1, second and third grid-stride passes, misaligned slices, extreme
logits, exact ties, zero probabilities, ignored and out-of-range labels.

Tolerance of every float comparison (``_check``): the same formula is evaluated
with fp32 torch on the CPU; its worst error against float64 is ``e32``; the
kernel's worst error must be <= 4 * e32 + 2 * ulp32(max |reference|), and never
looser than what tests/test_gpu_losses_and_module.py / test_gpu_backward.py
allow for the same quantity (``cap``).  The factor 4 is an allowance for another
summation order (wave tree, block partials, double final pass) and the device's
expf / logf, not a measurement; the measured ratio is printed per comparison.
Integers, argmax, power-of-two scalings and option combinations are exact.
``-m gpu``."""
import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import losses_numpy as LN

pytestmark = pytest.mark.gpu

W_SEM, W_DEPTH = 0.04, 0.1


def _abi(x):
    return float(np.float32(x))


# The C ABI carries Adam's hyperparameters as fp32: the float64 reference and the
# fp32 torch yardstick get the SAME values (0.99f = 0.99 + 9.5e-9), or they would
# evaluate another formula: 1 - beta2 differs by 9.5e-7 relative between the two
# readings, and so does the raw second moment (not v / (1 - beta2^t), which
# divides it out again: the parameters never see it).
ADAM = dict(lr=_abi(1e-2), b1=_abi(0.9), b2=_abi(0.99), eps=_abi(1e-15))


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    return _ops


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _check(name, got, ref64, ref32, cap=None):
    """max |got - ref64| <= min(4 e32 + 2 ulp32(max |ref64|), cap); NaNs (the
    reference's None / empty mean) must sit in the same places."""
    got, ref64, ref32 = (np.asarray(a, np.float64) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, name
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(ref32), nan), name
    if nan.all():
        return 0.0
    ok = ~nan
    peak = float(np.abs(ref64[ok]).max())
    e32 = float(np.abs(ref32[ok] - ref64[ok]).max())
    err = float(np.abs(got[ok] - ref64[ok]).max())
    bound = 4.0 * e32 + 2.0 * ulp32(peak)
    if cap is not None:
        bound = min(bound, cap)
    ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{name}: err {err:.3e} e32 {e32:.3e} err/e32 {ratio:.2f} bound {bound:.3e} peak {peak:.3e}")
    assert err <= bound, (name, err, e32, bound)
    return ratio


# ---------------------------------------------------------------------------
# ucsa_nerf_loss
# ---------------------------------------------------------------------------
def _nerf_args(case):
    return [_cu(case[k]) for k in ("rgb", "sem", "depth", "gt_rgb", "labels", "gt_depth")]


@pytest.mark.parametrize("N,C,kind", [(n, c, "plain") for n, c in LN.NERF_SHAPES] + LN.NERF_SPECIAL)
def test_nerf_loss_values_and_gradients(ops, N, C, kind):
    from ucsa_neural_rendering_amd import losses as ul
    case = LN.nerf_case(N, C, kind)
    ref_stats, ref_g = LN.nerf_loss_ref(case["rgb"], case["sem"], case["depth"], case["gt_rgb"],
                                        case["labels"], case["gt_depth"], case["uom"], W_SEM, W_DEPTH)
    # the fp32 yardstick; labels >= C go in as -1: torch raises on them where the
    # kernel's documented behaviour is to ignore them
    t32_stats, t32_g = LN.torch_nerf(case, torch.float32, W_SEM, W_DEPTH)
    args = _nerf_args(case)
    stats, g = ops.nerf_loss(*args, case["uom"], W_SEM, W_DEPTH, grad_scale=1.0)
    _, g128 = ops.nerf_loss(*args, case["uom"], W_SEM, W_DEPTH, grad_scale=128.0)
    stats_only, none = ops.nerf_loss(*args, case["uom"], W_SEM, W_DEPTH, want_grad=False)
    torch.cuda.synchronize()
    stats = _np(stats).astype(np.float64)
    assert none is None and np.array_equal(_np(stats_only), stats.astype(np.float32), equal_nan=True)
    assert stats[3] == ref_stats[3] and stats[4] == ref_stats[4] and stats[7] == 0.0
    tag = f"nerf[{N},{C},{kind}]"
    # existing bounds: 1e-6 abs colour / depth, 2e-6 rel semantics.  The relative one
    # only where the term is not ~0: with C = 1 every p_l is 1, the term is
    # -log(1 + 1e-15) = -1.1e-15 in float64 and exactly 0 in ANY fp32 evaluation
    # (1 + 1e-15 rounds to 1), so 2e-6 of it cannot be met; the derived bound
    # (4 e32 + 2 ulp, here ~5e-15) holds there on its own.
    rel = lambda x: 2e-6 * abs(x) if abs(x) > 2.0 ** -23 else None
    caps = {0: 1e-6, 1: rel(ref_stats[1]), 2: 1e-6, 5: 2e-6, 6: rel(ref_stats[6])}
    for k, cap in caps.items():
        _check(f"{tag} stats[{k}]", stats[k], ref_stats[k], t32_stats[k], cap=cap)
    if kind == "all_invalid":
        assert np.isnan(stats[1]) and stats[6] == 0.0 and not _np(g[1]).any()
    if kind == "no_depth":
        assert np.isnan(stats[2]) and np.isnan(stats[5]) and not _np(g[2]).any()
    # gradients.  A row whose labelled class has probability exactly 0 has a
    # finite gradient ~1e12 times the others (only the +1e-15 keeps it finite):
    # such rows are compared among themselves so that they do not hide the rest.
    huge = np.zeros(N, bool)
    huge[case["huge_rows"]] = kind != "all_invalid"
    for name, got, r64, r32 in zip(("d_rgb", "d_sem", "d_depth"), g, ref_g, t32_g):
        got = _np(got).astype(np.float64)
        if name == "d_sem":
            _check(f"{tag} d_sem", got[~huge], r64[~huge], r32[~huge],
                   cap=1e-6 * max(1.0, float(np.abs(r64[~huge]).max(initial=0))))
            if huge.any():
                assert np.isfinite(got[huge]).all() and np.abs(got[huge]).max() > 1e9 / N
                _check(f"{tag} d_sem zero-probability rows", got[huge], r64[huge], r32[huge],
                       cap=1e-6 * float(np.abs(r64[huge]).max()))
        else:
            _check(f"{tag} {name}", got, r64, r32, cap=1e-6 * max(1.0, float(np.abs(r64).max())))
    if case["zero_prob_row"] is not None and kind == "plain":
        assert huge[case["zero_prob_row"]]
    for a, b in zip(g128, g):
        assert torch.equal(a, b * 128.0)
    # the autograd route: the same kernel, so the same bits
    b = [x.clone().requires_grad_() for x in args[:3]]
    lc, ls, ld = ul.nerf_losses(b[0], b[1], b[2], args[3], args[4], args[5], case["uom"])
    ul.nerf_total_loss(lc, ls, ld).backward()
    f32 = stats.astype(np.float32)
    assert np.array_equal(_np(torch.stack([lc, ls, ld])), f32[[0, 6, 2]], equal_nan=True)
    for x, want in zip(b, g):
        assert torch.equal(x.grad, want.view(x.shape))


# ---------------------------------------------------------------------------
# ucsa_nerf_loss_apply
# ---------------------------------------------------------------------------
_COTANGENTS = {            # (total, colour, semantics, depth), no power of two among them
    "total": (1.7, None, None, None),
    "colour": (None, 0.3, None, None),
    "semantics": (None, None, -2.3, None),
    "depth": (None, None, None, 0.9),
    "all": (1.7, 0.3, -2.3, 0.9),
}


def _apply_and_check(ops, tag, grads, cot):
    saved = [x.clone() for x in grads]
    dev = [None if c is None else torch.tensor([c], device="cuda") for c in cot]
    out = ops.nerf_loss_apply(grads, *dev, W_SEM, W_DEPTH)
    torch.cuda.synchronize()
    for x, s in zip(grads, saved):
        assert torch.equal(x, s), "the saved gradients were written to"
    # the cotangents as the kernel receives them: fp32 values
    c32 = [None if c is None else float(np.float32(c)) for c in cot]
    ref = LN.nerf_loss_apply_ref([_np(x) for x in grads], *c32, W_SEM, W_DEPTH)
    z = lambda c: torch.tensor(0.0 if c is None else c, dtype=torch.float32)
    k32 = (z(cot[0]) + z(cot[1]), z(cot[0]) + z(cot[2]) / W_SEM, z(cot[0]) + z(cot[3]) / W_DEPTH)
    worst = 0.0
    for name, o, r, x, k in zip(("rgb", "sem", "depth"), out, ref, grads, k32):
        worst = max(worst, _check(f"apply[{tag}] {name}", _np(o), r, (x.cpu() * k).numpy()))
    return worst


@pytest.mark.parametrize("which", list(_COTANGENTS))
def test_nerf_loss_apply_cotangent_combinations(ops, which):
    case = LN.nerf_case(257, 40)
    _, grads = ops.nerf_loss(*_nerf_args(case), case["uom"], W_SEM, W_DEPTH)
    # without the ~1e12 row: it would set the scale of the whole comparison
    grads[1][case["huge_rows"]] = 0
    _apply_and_check(ops, which, grads, _COTANGENTS[which])


def test_nerf_loss_apply_three_grid_stride_passes(ops):
    """N (4 + C) = 2.2 M outputs against a grid capped at 4096 x 256 threads."""
    N, C = 50000, 40
    g = torch.Generator().manual_seed(11)
    grads = tuple(torch.randn(s, generator=g).cuda() for s in ((N, 3), (N, C), (N,)))
    assert N * (4 + C) > 2 * 4096 * 256
    _apply_and_check(ops, "total, N=50000", grads, _COTANGENTS["total"])


# ---------------------------------------------------------------------------
# ucsa_seg_tail
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,scale,kind", LN.SEG_CASES)
def test_seg_tail_values_and_gradients(ops, shape, scale, kind):
    x, labels = LN.seg_case(shape, scale, kind)
    ref = LN.seg_tail_ref(x, labels)
    # fp32 yardstick: F.softmax + CrossEntropyLoss(ignore_index=-1); labels >= C
    # go in as -1 (torch raises on them, the kernel ignores them by contract)
    t32 = LN.torch_seg(x, labels, torch.float32)
    xd, ld = _cu(x), _cu(labels)
    full = ops.seg_tail(xd, ld, want_prob=True, want_grad=True)
    torch.cuda.synchronize()
    tag = f"seg[{shape},{scale},{kind}]"
    # exact: logits on the 1/8 grid, ties included -- no pixel is excluded
    assert np.array_equal(_np(full["argmax"]), ref["argmax"])
    assert np.array_equal(t32["argmax"], ref["argmax"])
    _check(f"{tag} prob", _np(full["prob"]), ref["prob"], t32["prob"], cap=1e-6)
    _check(f"{tag} loss", float(full["loss"]), ref["loss"], t32["loss"], cap=2e-6)
    gmax = float(np.abs(ref["d_logits"]).max())
    _check(f"{tag} d_logits", _np(full["d_logits"]), ref["d_logits"], t32["d_logits"],
           cap=1e-9 + 1e-5 * gmax)
    if kind == "all_ignored":
        assert float(full["loss"]) == 0.0 and not _np(full["d_logits"]).any()
    # options: whatever is still returned has the same bits
    for kw, lab in ((dict(want_prob=False, want_grad=True), ld), (dict(want_prob=True, want_grad=False), ld),
                    (dict(want_prob=True, want_grad=True), None), (dict(want_prob=False), None)):
        r = ops.seg_tail(xd, lab, **kw)
        assert (r["prob"] is None) == (not kw["want_prob"])
        assert (r["loss"] is None) == (lab is None)
        assert (r["d_logits"] is None) == (lab is None or not kw.get("want_grad", False))
        for k, v in r.items():
            if v is not None:
                assert torch.equal(v, full[k]), (kw, k)
    r64 = ops.seg_tail(xd, ld, grad_scale=64.0, want_prob=False, want_grad=True)
    # a power-of-two scale is exact wherever the unscaled result is a normal fp32
    # number; at logit scale 80 some gradients are subnormal (p ~ e^-100), and
    # there the scaled run keeps bits that the unscaled one rounded (or flushed) away
    g1, g64 = full["d_logits"], r64["d_logits"]
    normal = g1.abs() >= 2.0 ** -126
    assert torch.equal(g64[normal], g1[normal] * 64.0)
    if not bool(normal.all()):            # zeros (ignored pixels) and subnormals
        assert float((g64[~normal] - g1[~normal] * 64.0).abs().max()) <= 64.0 * 2.0 ** -126
    assert torch.equal(r64["loss"], full["loss"])


@pytest.mark.parametrize("form", ["bf16", "channels_last"])
def test_seg_loss_on_bf16_and_channels_last_logits(ops, form):
    from ucsa_neural_rendering_amd import losses as ul
    x, labels = LN.seg_case((2, 40, 17, 23), 3, "random")
    ld = _cu(labels)
    if form == "bf16":
        xin = _cu(x).to(torch.bfloat16)
    else:
        xin = _cu(x).contiguous(memory_format=torch.channels_last)
        assert not xin.is_contiguous()
    plain = xin.detach().float().contiguous().requires_grad_()
    want = ul.seg_loss(plain, ld)
    want.backward()
    xin.requires_grad_()
    got = ul.seg_loss(xin, ld)
    got.backward()
    assert torch.equal(got.detach(), want.detach())
    assert xin.grad.shape == xin.shape and xin.grad.dtype == xin.dtype
    assert torch.equal(xin.grad, plain.grad.to(xin.dtype))
    assert float(plain.grad.abs().max()) > 0


# ---------------------------------------------------------------------------
# ucsa_semantic_postproc
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("C", [1, 2, 40, 64])
def test_semantic_postproc_ties_zero_rows_and_tiny_sums(ops, N, C):
    s = LN.postproc_case(N, C)
    scales = (1.0, 2.0 ** -100) if (N, C) == (257, 40) else (1.0,)
    for scale in scales:
        x = s * np.float32(scale)            # exact; the sums are tiny but not 0
        ref_n, ref_a = LN.semantic_postproc_ref(x)
        t32_n, t32_a = ol.semantic_postproc(torch.from_numpy(x))
        n, a = ops.semantic_postproc(_cu(x))
        none, a2 = ops.semantic_postproc(_cu(x), want_normalised=False)
        torch.cuda.synchronize()
        # exact, no row excluded: entries on the 1/1024 grid tie exactly or not at all
        assert np.array_equal(_np(a), ref_a) and np.array_equal(t32_a.numpy(), ref_a)
        assert none is None and torch.equal(a2, a)
        _check(f"postproc[{N},{C},{scale:g}]", _np(n), ref_n, t32_n.numpy(), cap=1e-7)
        if scale != 1.0:
            assert np.array_equal(_np(n), _np(ops.semantic_postproc(_cu(s))[0]))


# ---------------------------------------------------------------------------
# ucsa_confusion_matrix
# ---------------------------------------------------------------------------
N_CONF_BIG = 2 * 2048 * 256 + 77          # two full passes of the capped grid and a tail


@pytest.mark.parametrize("n,C", [(1, 1), (1, 40), (255, 1), (255, 41), (N_CONF_BIG, 40),
                                 (N_CONF_BIG, 41)])
def test_confusion_matrix_sizes_and_out_of_range_values(ops, n, C):
    assert N_CONF_BIG == 1048653
    p, t = LN.confusion_case(n, C)
    cm = ops.confusion_matrix(_cu(p), _cu(t), C)
    want = LN.confusion_ref(p, t, C)
    assert cm.dtype == torch.int64 and np.array_equal(_np(cm), want)
    assert want.sum() <= n and (n < 255 or want.sum() < n)


def test_confusion_matrix_one_hot_cell_and_accumulation(ops):
    n, C = N_CONF_BIG, 40
    cm = ops.confusion_matrix(torch.full((n,), 3, device="cuda"), torch.full((n,), 7, device="cuda"), C)
    want = np.zeros((C, C), np.int64)
    want[7, 3] = n
    assert np.array_equal(_np(cm), want)
    # into a pre-filled matrix, across two calls
    p, t = LN.confusion_case(n, C, seed=1)
    cm0 = np.random.default_rng(5).integers(0, 2 ** 40, size=(C, C))
    cm = _cu(cm0.copy())
    h = n // 2 + 1
    assert ops.confusion_matrix(_cu(p[:h]), _cu(t[:h]), C, cm=cm) is cm
    ops.confusion_matrix(_cu(p[h:]), _cu(t[h:]), C, cm=cm)
    assert np.array_equal(_np(cm), LN.confusion_ref(p, t, C, cm0=cm0))


# ---------------------------------------------------------------------------
# ucsa_adam_step
# ---------------------------------------------------------------------------
N_ADAM_BIG = 2 * 2048 * 256 * 4 + 3       # three grid-stride passes of k_adam and a scalar tail


def _torch_adam32(p0, wd):
    p = torch.from_numpy(p0.copy()).requires_grad_()
    return p, torch.optim.Adam([p], lr=ADAM["lr"], betas=(ADAM["b1"], ADAM["b2"]),
                               eps=ADAM["eps"], weight_decay=wd)


def _check_adam(tag, dev, ref, opt_p, opt):
    st = opt.state[opt_p]
    t32 = (opt_p.detach(), st["exp_avg"], st["exp_avg_sq"])
    # existing bound: 2e-6 on the parameters
    for name, d, r, t, cap in zip("pmv", dev, ref, t32, (2e-6, None, None)):
        _check(f"{tag} {name}", _np(d), r, t.numpy(), cap=cap)


def _adam_run(ops, n, wd, offset=0):
    """Three steps on [offset, offset + n) of buffers with guard floats on both
    sides; gradients arrive scaled by 8 and are unscaled by inv_grad_scale."""
    rng = np.random.default_rng(n + int(wd * 1e7))
    wd = _abi(wd)
    pad = 8
    p0 = rng.standard_normal(n).astype(np.float32)
    guard = [torch.from_numpy(rng.standard_normal(n + 2 * pad).astype(np.float32)).cuda()
             for _ in range(4)]
    sl = slice(pad + offset, pad + offset + n)
    p, g, m, v = (b[sl] for b in guard)
    p.copy_(torch.from_numpy(p0))
    m.zero_()
    v.zero_()
    before = [b.clone() for b in guard]
    ref = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    tp, opt = _torch_adam32(p0, wd)
    for step in (1, 2, 3):
        grad = LN.adam_grads(rng, n)
        g.copy_(torch.from_numpy(grad * np.float32(8.0)))
        ops.adam_step(p, g, m, v, step, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd,
                      inv_grad_scale=1.0 / 8.0)
        ref = LN.adam_ref(*ref[:1], grad, *ref[1:], step, ADAM["lr"], ADAM["b1"], ADAM["b2"],
                          ADAM["eps"], wd)
        tp.grad = torch.from_numpy(grad.copy())
        opt.step()
        torch.cuda.synchronize()
        _check_adam(f"adam[n={n},wd={wd:g},off={offset}] step {step}", (p, m, v), ref, tp, opt)
    for b, b0, name in zip(guard, before, "pgmv"):
        if name != "g":
            assert torch.equal(b[:sl.start], b0[:sl.start]) and torch.equal(b[sl.stop:], b0[sl.stop:]), \
                f"{name}: written outside the slice"


@pytest.mark.parametrize("wd", [0.0, 1e-6])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025])
def test_adam_step_p_m_v_small_sizes(ops, n, wd):
    _adam_run(ops, n, wd)


@pytest.mark.parametrize("wd,offset", [(0.0, 0), (1e-6, 0), (1e-6, 1)])
def test_adam_step_p_m_v_grid_stride_passes(ops, wd, offset):
    """offset 1: the slice starts 4 bytes off a 16-byte boundary, i.e. the scalar
    path at grid-stride size (the sharded optimizer hands over such slices)."""
    assert N_ADAM_BIG == 4194307
    _adam_run(ops, N_ADAM_BIG, wd, offset)


# ---------------------------------------------------------------------------
# ucsa_adam_step_scaled / ucsa_adam_count_skipped
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 2 * 4096 * 256 + 5])
def test_adam_step_scaled_skips_without_counting(ops, n):
    rng = np.random.default_rng(n)
    wd, scale = _abi(1e-6), 1024.0
    found = [0.0, 1.0, 0.0, 0.0]
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [LN.adam_grads(rng, n) for _ in found]
    hist, n_skipped = LN.adam_scaled_ref(p0, [g.astype(np.float64) * scale for g in grads],
                                         np.zeros(n), np.zeros(n), found, [scale] * 4,
                                         ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd)
    assert n_skipped == 1
    p, m, v = _cu(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    skipped = torch.zeros(1, dtype=torch.int32, device="cuda")
    gs = torch.tensor([scale], device="cuda")
    tp, opt = _torch_adam32(p0, wd)
    for step, (grad, fi) in enumerate(zip(grads, found), 1):
        fi_d = torch.tensor([fi], device="cuda")
        g = _cu(grad * np.float32(scale))
        if fi:
            g[::3] = float("inf")
        before = [x.clone() for x in (p, m, v)]
        ops.adam_step_scaled(p, g, m, v, step, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], wd,
                             gs, fi_d, skipped)
        ops.adam_count_skipped(fi_d, skipped)
        torch.cuda.synchronize()
        if fi:
            assert all(torch.equal(a, b) for a, b in zip((p, m, v), before))
            assert int(skipped[0]) == 1
        else:
            tp.grad = torch.from_numpy(grad.copy())      # torch's own count skips with it
            opt.step()
            _check_adam(f"adam_scaled[n={n}] step {step}", (p, m, v), hist[step - 1], tp, opt)
    assert int(skipped[0]) == 1

