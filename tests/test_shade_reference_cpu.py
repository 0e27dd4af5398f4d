"""The float64 yardstick of the colour / semantics / compositing stage
(tests/shade_numpy.py) held against the oracle and against itself, on the CPU:

* it agrees with ``oracle.renderer`` / ``oracle.field`` and their autograd, in
  float64 where the oracle's pieces allow it and in fp32 (``fld.color`` /
  ``fld.semantics`` as ``run`` calls them) within the fp32 bounds, plain and
  fp16-emulating;
* a plain fp32 numpy evaluation of the same formulas, sequential sums, stays
  inside the fp32 bounds: they are not tighter than the arithmetic allows;
* every deliberately wrong reference is rejected by the very ``compare_*``
  calls the GPU tests use;
* every case the GPU tests run stays under the 5 % redraw cap at the fp32,
  f16 and bf16x2 margins, by the reference alone.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import field as ofield
from oracle import renderer as oren
from tests import shade_numpy as sn
from tests.util import lively_oracle_field

F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _field(C):
    return lively_oracle_field(C=C)


@functools.lru_cache(maxsize=None)
def _case(family, mode_name="fp32", **kw):
    mode = {str(m): m for m in sn.PIN_MODES}[mode_name]
    fld = _field(kw.get("C", 40))
    return sn.build_case(family, fld.color_params.numpy(), fld.sem_params.numpy(), mode, **kw)


def _both(c, mode=sn.FP32, dt=F64, mutant=(), weights=None):
    fw = sn.composite_forward(*sn.forward_args(c), mode=mode, dt=dt, mutant=mutant)
    w = np.asarray(fw.weights, F32) if weights is None else weights
    bw = sn.composite_backward(*sn.forward_args(c), fw.src, w, c.d_image, c.d_depth,
                               c.d_sem, mode=mode, dt=dt, mutant=mutant)
    return fw, bw


def _fwd_dict(r):
    return {k: getattr(r, k) for k in ("src", "weights", "image", "depth", "semantics")}


def _bwd_dict(r):
    return {k: getattr(r, k) for k in ("G", "d_h_c", "d_h_f", "dW_color", "dW_sem")}


# ---------------------------------------------------------------------------
# the oracle's stage on the same inputs, by autograd
# ---------------------------------------------------------------------------
def oracle_stage(c, dtype, emulate_fp16=False):
    """renderer.run from the merge on (:113-146) on explicit stage inputs.
    float64: the oracle's ``alpha_weights``, ``sh4_encode``, ``mlp_forward``
    under the masked scatter of ``color`` / ``semantics`` (those two methods
    build fp32 buffers); float32: ``fld.color`` / ``fld.semantics`` themselves.
    sigma = trunc_exp(h0) in fp32 (``_TruncExp`` computes in fp32)."""
    N, T, t, C = c.N, c.T, c.t, c.C
    fld = _field(C)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    h_all = tt(sn._rows(c.h_c, c.h_f, N, T, t))                       # [N, S, 16] fp32
    h0 = h_all[..., 0].clone().requires_grad_()
    geo = h_all[..., 1:].to(dtype).clone().requires_grad_()
    cp = fld.color_params.to(dtype).clone().requires_grad_()
    sp = fld.sem_params.to(dtype).clone().requires_grad_()
    rays_d = tt(c.rays_d).to(dtype).requires_grad_()                  # (grad: keeps _q16 in dtype)
    sigma32 = ofield.trunc_exp(h0)
    z = tt(c.z_c if t == 0 else np.concatenate([c.z_c, c.z_f], 1)).to(dtype)
    zs, order = torch.sort(z, dim=1, stable=True)
    sg = torch.gather(sigma32.to(dtype), 1, order)
    geo_s = torch.gather(geo, 1, order.unsqueeze(-1).expand(-1, -1, 15))
    _, weights = oren.alpha_weights(zs, sg, c.density_scale)
    mask = weights > 1e-4
    S = T + t
    dirs = rays_d.view(-1, 1, 3).expand(N, S, 3).reshape(-1, 3)
    flat_geo, m = geo_s.reshape(N * S, 15), mask.reshape(-1)
    if dtype == torch.float32:
        # emulate_fp16: True = the field's flag, "nets" = per net (emulate_fp16_nets)
        f2 = ofield.OracleField(num_semantic_classes=C, seed=None, emulate_fp16=emulate_fp16 is True)
        if emulate_fp16 == "nets":
            f2.emulate_fp16_nets = ("color", "sem")
        f2.color_params, f2.sem_params = cp, sp
        rgbs = f2.color(None, dirs, mask=m, geo_feat=flat_geo).view(N, S, 3)
        probs = f2.semantics(None, dirs, mask=m, geo_feat=flat_geo).view(N, S, C)
    else:
        rgbs = torch.zeros(N * S, 3, dtype=dtype)
        probs = torch.zeros(N * S, C, dtype=dtype)
        if m.any():
            x = torch.cat([ofield.sh4_encode((dirs[m] + 1) / 2), flat_geo[m]], -1)
            rgbs = rgbs.index_put((m.nonzero()[:, 0],), torch.sigmoid(
                ofield.mlp_forward(fld.color_spec, x, cp, emulate_fp16)))
            probs = probs.index_put((m.nonzero()[:, 0],), torch.softmax(
                ofield.mlp_forward(fld.sem_spec, flat_geo[m], sp, emulate_fp16), -1))
        rgbs, probs = rgbs.view(N, S, 3), probs.view(N, S, C)
    w_sem = torch.where(mask, weights.detach(), torch.zeros_like(weights))
    w_rgb = torch.where(mask, weights, torch.zeros_like(weights))
    depth = torch.sum(w_rgb * zs, -1) / tt(c.norms).to(dtype)
    image = torch.sum(w_rgb.unsqueeze(-1) * rgbs, -2)
    sem = torch.sum(w_sem.unsqueeze(-1) * probs, -2)
    ((image * tt(c.d_image).to(dtype)).sum() + (depth * tt(c.d_depth).to(dtype)).sum()
     + (sem * tt(c.d_sem).to(dtype)).sum()).backward()
    d_h = torch.cat([h0.grad.to(dtype).unsqueeze(-1), geo.grad], -1)
    # G = dL/dw of the colour / depth path, from the same tensors
    out = dict(src=order.numpy().astype(np.int32), weights=weights.detach().numpy(),
               image=image.detach().numpy(), depth=depth.detach().numpy(),
               semantics=sem.detach().numpy(),
               d_h_c=d_h[:, :T].reshape(N * T, 16).numpy(),
               d_h_f=d_h[:, T:].reshape(N * t, 16).numpy() if t else None,
               dW_color=cp.grad.numpy(), dW_sem=sp.grad.numpy(),
               sigma_c=sigma32.detach().numpy()[:, :T],
               sigma_f=sigma32.detach().numpy()[:, T:] if t else None)
    return out


ORACLE_CASES = [("tails", dict(N=3)), ("blocks", {}), ("long", dict(T=33, t=32)),
                ("weights", {}), ("classes", dict(C=17)), ("classes", dict(C=1)), ("t0", {})]


def _with_oracle_sigma(c, o):
    """the case with sigma = fp32 trunc_exp(h0), the value the oracle's graph holds"""
    import copy
    c = copy.copy(c)
    c.sigma_c, c.sigma_f = o["sigma_c"].astype(F32), None if c.t == 0 else o["sigma_f"].astype(F32)
    return c


@pytest.mark.parametrize("family,kw", ORACLE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("emulate", [False, True], ids=["plain", "fp16emu"])
def test_reference_matches_oracle_autograd_in_float64(family, kw, emulate):
    """Two float64 evaluations of the same mathematics: plain, they agree to 2^-20 of
    the fp32 budget of every element (the budget has the conditioning of the
    element in it: float64 noise is 2^-29 of it).  Slot 0 passes the oracle's
    fp32 ``_TruncExp.backward``: one fp32 product and the cast of its input."""
    c = _case(family, **kw)
    o = oracle_stage(c, torch.float64, emulate)
    c = _with_oracle_sigma(c, o)
    mode = sn.F16M(1.0, round_grads=False) if emulate else sn.FP32
    fw = sn.composite_forward(*sn.forward_args(c), mode=mode)
    bw = sn.composite_backward(*sn.forward_args(c), fw.src, fw.weights, c.d_image, c.d_depth,
                               c.d_sem, mode=mode)
    # fp16-emulating: torch rounds double -> half through float, a double
    # rounding that moves a value sitting within 2^-25 of a tie to the other
    # side; the fp16 mode's own bounds flag exactly those elements (one fp16
    # ulp where a boundary is within the fp32 budget) and are fp32-grade
    # elsewhere -- a misplaced quantisation is 2^-11, far above them
    tight = 1.0 if emulate else 2.0 ** -20
    floor = lambda ref, e: np.where(np.isfinite(e), e * tight, np.inf) + 1e-13 * np.abs(ref) + 1e-300
    sn.compare_exact(o["src"], fw.src, "src")
    e_fp32 = fw if emulate else sn.composite_forward(*sn.forward_args(c), mode=sn.FP32)
    for k in ("weights", "image", "depth", "semantics"):
        sn.compare(o[k], getattr(fw, k), floor(getattr(fw, k), getattr(e_fp32, "e_" + k)), f"oracle64 {k}")
    e32 = bw if emulate else sn.composite_backward(*sn.forward_args(c), fw.src, fw.weights, c.d_image,
                                                   c.d_depth, c.d_sem, mode=sn.FP32)
    for k in ("d_h_c", "d_h_f", "dW_color", "dW_sem"):
        ref = getattr(bw, k)
        if ref is None:
            continue
        b = floor(ref, getattr(e32, "e_" + k))
        if k.startswith("d_h"):
            b[:, 0] = b[:, 0] + 4.0 * sn.U * np.abs(ref[:, 0])
        sn.compare(o[k], ref, b, f"oracle64 {k}")


@pytest.mark.parametrize("family,kw", ORACLE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("emulate", [False, True, "nets"], ids=["plain", "fp16emu", "fp16emu-nets"])
def test_oracle_fp32_methods_stay_within_the_fp32_bounds(family, kw, emulate):
    """``fld.color`` / ``fld.semantics`` / ``alpha_weights`` exactly as ``run``
    calls them, in fp32 with BLAS sums and torch's autograd, against the
    float64 reference within the fp32 bounds.  (The backward is fed the
    oracle's own fp32 weights, as an entry point would be.)  fp16-emulating:
    ``OracleField(emulate_fp16=True)`` and ``emulate_fp16_nets`` against the
    fp16 mode with its gradients unrounded (the oracle's casts are straight
    through), on the case pinned at the f16 margin."""
    mode = sn.F16M(1.0, round_grads=False) if emulate else sn.FP32
    c = _case(family, "f16(gs=1024)" if emulate else "fp32", **kw)
    o = oracle_stage(c, torch.float32, emulate)
    c = _with_oracle_sigma(c, o)
    fw = sn.composite_forward(*sn.forward_args(c), mode=mode)
    assert np.array_equal(fw.mask, o["weights"] > F32(1e-4)), "mask not pinned"
    sn.compare_forward({k: o[k] for k in ("src", "weights", "image", "depth", "semantics")},
                       fw, "oracle32")
    bw = sn.composite_backward(*sn.forward_args(c), o["src"], o["weights"], c.d_image,
                               c.d_depth, c.d_sem, mode=mode)
    # autograd differentiates ITS fp32 weights' graph: cumprod's backward is
    # not the kernel's scan, but it is fp32 arithmetic on the same sums
    sn.compare_backward({k: o[k] for k in ("d_h_c", "d_h_f", "dW_color", "dW_sem")}, bw, "oracle32")


@pytest.mark.parametrize("M", [1, 17, 257])
@pytest.mark.parametrize("h16", [False, True])
def test_sigma_backward_matches_oracle_autograd(M, h16):
    fld = _field(40)
    c = sn.build_sigma_case(fld.sigma_params.numpy(), M)
    ref = sn.sigma_backward(c.feat, c.d_h, c.sigma_params, round_hidden=h16)
    for dtype in (torch.float64, torch.float32):
        p = fld.sigma_params.to(dtype).clone().requires_grad_()
        x = torch.from_numpy(c.feat).to(dtype).requires_grad_()
        W1, W2 = ofield.mlp_split(fld.sigma_spec, p)
        if h16:     # the hidden layer rounded to fp16, gradients straight through
            y = torch.relu(ofield._q16(x @ W1.t())) @ W2.t()
        else:
            y = ofield.mlp_forward(fld.sigma_spec, x, p)
        (y * torch.from_numpy(c.d_h).to(dtype)).sum().backward()
        got = dict(d_feat=x.grad.numpy(), dW=p.grad.numpy())
        if dtype == torch.float32:
            sn.compare_sigma(got, ref, f"sigma oracle32 M={M}")
        else:
            for k in got:
                # (h16: torch's double -> float -> half double rounding, see above)
                sn.compare(got[k], getattr(ref, k), getattr(ref, "e_" + k) * (1.0 if h16 else 2.0 ** -20)
                           + 1e-13 * np.abs(getattr(ref, k)) + 1e-300, f"sigma oracle64 {k}")


# ---------------------------------------------------------------------------
# the bounds are not tighter than fp32 arithmetic allows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,kw", [("tails", dict(N=17)), ("blocks", {}), ("long", dict(T=96, t=34)),
                                       ("weights", {}), ("classes", dict(C=61)), ("t0", {})],
                         ids=lambda v: str(v))
def test_plain_fp32_numpy_stays_inside_the_fp32_bounds(family, kw):
    c = _case(family, **kw)
    fw, bw = _both(c)
    fw32, bw32 = _both(c, dt=F32, weights=np.asarray(fw.weights, F32))
    assert fw32.weights.dtype == F32 and bw32.d_h_c.dtype == F32 and bw32.dW_color.dtype == F32
    sn.compare_forward(_fwd_dict(fw32), fw, "numpy32")
    sn.compare_backward(_bwd_dict(bw32), bw, "numpy32")


@pytest.mark.parametrize("M", [17, 257])
def test_plain_fp32_numpy_sigma_backward_stays_inside_the_bounds(M):
    c = sn.build_sigma_case(_field(40).sigma_params.numpy(), M)
    ref = sn.sigma_backward(c.feat, c.d_h, c.sigma_params)
    got = sn.sigma_backward(c.feat, c.d_h, c.sigma_params, dt=F32)
    assert got.d_feat.dtype == F32
    sn.compare_sigma(dict(d_feat=got.d_feat, dW=got.dW), ref, "numpy32 sigma")


# ---------------------------------------------------------------------------
# sharpness: each wrong reference is rejected by the GPU tests' compare calls
# ---------------------------------------------------------------------------
MUTANT_CASES = {
    "next_ray_dimage": ("blocks", {}, "bwd"),
    "tail_shift": ("blocks", {}, "bwd"),
    "sem_not_detached": ("tails", dict(N=3), "bwd"),
    "drop_1e15": ("weights", {}, "bwd"),
    "last_delta_prev": ("tails", dict(N=3), "fwd"),
    "no_clamp": ("weights", {}, "bwd"),
    "suffix_inclusive": ("tails", dict(N=3), "bwd"),
    "carry_lost_64": ("long", dict(T=96, t=34), "bwd"),
    "softmax_padded": ("classes", dict(C=17), "fwd"),
    "unstable_merge": ("weights", {}, "fwd"),
    "depth_no_norm": ("tails", dict(N=3), "fwd"),
}


def test_every_mutant_has_a_case():
    assert set(MUTANT_CASES) | {"gate_ge"} == set(sn.MUTANTS)


@pytest.mark.parametrize("mode_name", ["fp32", "bf16x2", "f16(gs=1024)"])
@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_wrong_references_are_rejected(mutant, mode_name):
    family, kw, where = MUTANT_CASES[mutant]
    c = _case(family, mode_name, **kw)
    mode = {str(m): m for m in sn.PIN_MODES}[mode_name]
    fw, bw = _both(c, mode)
    # the right reference passes its own comparison ...
    sn.compare_forward(_fwd_dict(fw), fw, "self")
    sn.compare_backward(_bwd_dict(bw), bw, "self")
    # ... the wrong one does not (the backward is fed the RIGHT src / weights,
    # as the GPU test feeds the kernel)
    bad_fw = sn.composite_forward(*sn.forward_args(c), mode=mode, mutant=(mutant,))
    if where == "fwd":
        with pytest.raises(sn.Mismatch):
            sn.compare_forward(_fwd_dict(bad_fw), fw, mutant)
    else:
        bad_bw = sn.composite_backward(*sn.forward_args(c), fw.src, np.asarray(fw.weights, F32),
                                       c.d_image, c.d_depth, c.d_sem, mode=mode, mutant=(mutant,))
        with pytest.raises(sn.Mismatch):
            sn.compare_backward(_bwd_dict(bad_bw), bw, mutant)


def test_carry_lost_is_caught_in_the_forward_too():
    c = _case("long", T=96, t=34)
    fw = sn.composite_forward(*sn.forward_args(c))
    bad = sn.composite_forward(*sn.forward_args(c), mutant=("carry_lost_64",))
    with pytest.raises(sn.Mismatch):
        sn.compare_forward(_fwd_dict(bad), fw, "carry")


@pytest.mark.parametrize("mode,h16", [(sn.FP32, False), (sn.X2, False), (sn.FP32, True)])
def test_gate_at_exact_zero_is_rejected_when_open(mode, h16):
    """A feat row of zeros gives every hidden unit the pre-activation 0 exactly
    (no bias): ``>`` closes the gate, ``>=`` lets W1^T W2^T d_h through."""
    c = sn.build_sigma_case(_field(40).sigma_params.numpy(), 17)
    ref = sn.sigma_backward(c.feat, c.d_h, c.sigma_params, mode, h16)
    sn.compare_sigma(dict(d_feat=ref.d_feat, dW=ref.dW), ref, "self")
    bad = sn.sigma_backward(c.feat, c.d_h, c.sigma_params, mode, h16, mutant=("gate_ge",))
    with pytest.raises(sn.Mismatch):
        sn.compare_sigma(dict(d_feat=bad.d_feat, dW=bad.dW), ref, "gate_ge")


# ---------------------------------------------------------------------------
# the redraw cap, by the reference alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", ["fp32", "bf16x2", "f16(gs=1024)"])
def test_every_gpu_case_stays_under_the_redraw_cap(mode_name):
    for family, key, kw in sn.all_case_specs():
        c = _case(family, mode_name, **kw)
        print(f"{c.name} at the {mode_name} margin: {c.redrawn:.1%} redrawn (seed attempt {c.reseeded})")
        assert c.redrawn <= 0.05
        fw = sn.composite_forward(*sn.forward_args(c))
        gap = np.abs(fw.weights - sn.W_MIN) - fw.e_weights
        assert (gap > 0).all(), "a weight within its bound of the mask threshold"


def test_every_sigma_case_stays_under_the_redraw_cap():
    for M in sn.SIGMA_M:
        c = sn.build_sigma_case(_field(40).sigma_params.numpy(), M)
        assert c.redrawn <= 0.05
        assert (c.d_h == 0).all(1).sum() >= (M >= 64), "zero d_h rows"
