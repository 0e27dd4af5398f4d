"""The colour / semantics / compositing entry points and the sigma-net backward
against the float64 reference of tests/shade_numpy.py, element by element,
within bounds derived there from counting rounding steps: one test id = one
entry point on one case.  Inputs are synthetic stage inputs (no hash grid, no
render), pinned by the builders so that no ReLU gate and no mask decision lies
within the kernel's error of its threshold: there are no exempt samples and no
L2 fallback.  tests/test_shade_reference_cpu.py holds the reference against the
oracle and shows that the same ``compare_*`` calls reject wrong references.

Worst err / bound per entry point and case family, as printed at the end of a
run on an MI355X: docs/DESIGN_NOTEBOOK.md, "Float64 per-sample parity of the
shading stage"."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import shade_numpy as sn
from tests.util import lively_oracle_field

pytestmark = pytest.mark.gpu
F32 = np.float32
MODES = {str(m): m for m in sn.PIN_MODES}


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    yield _ops
    if sn.WORST:
        print("\nworst err / bound per entry point, case family and output:")
        for k in sorted(sn.WORST):
            print(f"  {k}: {sn.WORST[k]:.3f}")


@functools.lru_cache(maxsize=None)
def _field(C):
    return lively_oracle_field(C=C)


@functools.lru_cache(maxsize=None)
def _case(family, key, pin):
    args = next(a for f, k, a in sn.all_case_specs() if f == family and k == key)
    fld = _field(args.get("C", 40))
    return sn.build_case(family, fld.color_params.numpy(), fld.sem_params.numpy(), MODES[pin], **args)


@functools.lru_cache(maxsize=None)
def _ref_forward(family, key, pin, mode_name):
    c = _case(family, key, pin)
    mode = {"fp32": sn.FP32, "f16": sn.F16M(1024.0), "x3": sn.X3, "h2": sn.H2}[mode_name]
    return sn.composite_forward(*sn.forward_args(c), mode=mode)


@functools.lru_cache(maxsize=None)
def _ref_backward(family, key, pin, mode_name, gs):
    c = _case(family, key, pin)
    mode = {"fp32": sn.FP32, "f16": sn.F16M(gs), "x2": sn.X2}[mode_name]
    fw = _ref_forward(family, key, pin, "fp32")
    w32 = np.asarray(fw.weights, F32)
    return fw.src, w32, sn.composite_backward(*sn.forward_args(c), fw.src, w32, c.d_image,
                                              c.d_depth, c.d_sem, mode=mode)


CASES = [(f, k) for f, k, _ in sn.all_case_specs()]
case_id = lambda v: v[0] if v[1] is None else v[0] + ("x".join(map(str, v[1])) if isinstance(v[1], tuple) else str(v[1]))


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _stage(c):
    return [_dev(a) for a in (c.rays_d, c.norms, c.z_c, c.sigma_c, c.h_c, c.z_f, c.sigma_f, c.h_f)]


# ---------------------------------------------------------------------------
# forwards
# ---------------------------------------------------------------------------
FWD = {"composite_fwd": ("fp32", "fp32"), "composite_fwd_f16": ("f16(gs=1024)", "f16"),
       "composite_train_fwd_x3": ("fp32", "x3"), "composite_train_fwd_h2": ("fp32", "h2")}


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("entry", list(FWD))
def test_forward(ops, entry, case):
    """src exactly; weights, image, depth, semantics within their bounds (the
    _x3 / _h2 forms against the non-emulated reference: they are fp32-grade)."""
    from ucsa_neural_rendering_amd import _lib
    pin, mode = FWD[entry]
    c = _case(*case, pin)
    ref = _ref_forward(*case, pin, mode)
    cp, sp = _dev(c.color_params), _dev(c.sem_params)
    a = _stage(c)
    if entry == "composite_fwd":
        out = ops.composite_fwd(*a, ops.mlp_pack(_lib.MLP_COLOR, cp, c.C), ops.mlp_pack(_lib.MLP_SEM, sp, c.C),
                                c.C, c.density_scale, want_aux=True)
    elif entry == "composite_fwd_f16":
        out = ops.composite_fwd(*a, ops.mlp_pack_f16(_lib.MLP_COLOR, cp, c.C),
                                ops.mlp_pack_f16(_lib.MLP_SEM, sp, c.C), c.C, c.density_scale,
                                want_aux=True, half=True)
    elif entry == "composite_train_fwd_x3":
        out = ops.composite_train_fwd_x3(*a, ops.mlp_pack_x3(_lib.MLP_COLOR, cp, c.C),
                                         ops.mlp_pack_x3(_lib.MLP_SEM, sp, c.C), c.C, c.density_scale)
    else:
        out = ops.composite_train_fwd_x3(*a, ops.mlp_pack_h2(_lib.MLP_COLOR, cp, c.C),
                                         ops.mlp_pack_h2(_lib.MLP_SEM, sp, c.C), c.C, c.density_scale, h2=True)
    torch.cuda.synchronize()
    image, depth, sem, src, w = out
    sn.compare_forward(dict(src=src, weights=w, image=image, depth=depth, semantics=sem), ref,
                       f"{entry} {case[0]}", c.name)


# the split inference composite (csrc/composite_split.hip: k_weights_compact +
# k_shade_dense / k_shade16): what every inference render runs
INFER = {"composite_infer": ("fp32", "fp32", "mlp_pack"),
         "composite_infer_f16": ("f16(gs=1024)", "f16", "mlp_pack_f16"),
         "composite_infer_x3": ("fp32", "x3", "mlp_pack_x3"),
         "composite_infer_h2": ("fp32", "h2", "mlp_pack_h2")}


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("entry", list(INFER))
def test_infer_forward(ops, entry, case):
    """image, depth and semantics of the kernel pair within their bounds,
    against the reference of the entry point's arithmetic.  The outputs start
    as NaN: a ray without a masked sample must still get its zeros.
    k_weights_compact decides the mask on its own fp32 weights, so the cases
    carry the same pin as for the fused forwards (no weight within its bound
    of 1e-4)."""
    from ucsa_neural_rendering_amd import _lib
    lib = _lib.lib()
    pin, mode, pack = INFER[entry]
    c = _case(*case, pin)
    ref = _ref_forward(*case, pin, mode)
    pc = getattr(ops, pack)(_lib.MLP_COLOR, _dev(c.color_params), c.C)
    ps = getattr(ops, pack)(_lib.MLP_SEM, _dev(c.sem_params), c.C)
    N, T, t = c.N, c.T, c.t
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    image, depth, sem = nan(N, 3), nan(N), nan(N, c.C)
    ws = torch.empty(max(16, int(lib.ucsa_composite_infer_workspace_bytes(N, T, t))),
                     dtype=torch.uint8, device="cuda")
    p = ops._ptr
    _lib.check(getattr(lib, "ucsa_" + entry)(
        *[p(v) for v in _stage(c)], p(pc), p(ps), N, T, t, c.C, float(c.density_scale),
        p(image), p(depth), p(sem), p(ws), ops._stream()), "ucsa_" + entry)
    torch.cuda.synchronize()
    sn.compare_forward(dict(image=image, depth=depth, semantics=sem), ref, f"{entry} {case[0]}", c.name)


# ---------------------------------------------------------------------------
# backwards
# ---------------------------------------------------------------------------
def _composite_bwd(ops, c, src, w32, kind, f16_scale):
    """ops.composite_bwd with every output and both partial buffers filled with
    NaN before the call (an idle wave must still write its zero partials, a
    sample outside the mask its zero G and d_h row) -> dict of outputs, dW
    reduced by ucsa_reduce_partials."""
    from ucsa_neural_rendering_amd import _lib
    lib = _lib.lib()
    N, T, t, Cn = c.N, c.T, c.t, c.C
    half, x2 = kind == "f16", kind == "x2"
    cp, sp = _dev(c.color_params), _dev(c.sem_params)
    if half:
        packs = (ops.mlp_pack_f16(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack_f16(_lib.MLP_SEM, sp, Cn),
                 ops.mlp_pack_t_f16(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack_t_f16(_lib.MLP_SEM, sp, Cn))
    elif x2:
        packs = (ops.mlp_pack_x3(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack_x3(_lib.MLP_SEM, sp, Cn),
                 ops.mlp_pack_t_x3(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack_t_x3(_lib.MLP_SEM, sp, Cn))
    else:
        packs = (ops.mlp_pack(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack(_lib.MLP_SEM, sp, Cn),
                 ops.mlp_pack_t(_lib.MLP_COLOR, cp, Cn), ops.mlp_pack_t(_lib.MLP_SEM, sp, Cn))
    a = _stage(c)
    src_d, w_d = _dev(src, torch.int32), _dev(w32)
    d_image, d_depth, d_sem = _dev(c.d_image), _dev(c.d_depth), _dev(c.d_sem)
    parts = int((lib.ucsa_composite_bwd_parts_f16 if half else lib.ucsa_composite_bwd_parts)(N))
    waves = 8 if ops.shade_bwd_split() else 4
    rpw = max(2, -(-N // (256 * waves)))
    assert parts == -(-(-(-N // rpw)) // waves) * waves, "partial slots: library and ops disagree"
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    nrb = (Cn + 15) // 16
    G, d_h_c = nan(N, T + t), nan(N * T, 16)
    d_h_f = nan(N * t, 16) if t else None
    pc, ps = nan(parts, 7168), nan(parts, 1024 + 1024 * nrb)
    p = ops._ptr
    head = [p(v) for v in a] + [p(src_d), p(w_d)] + [p(v) for v in packs] + \
           [p(d_image), p(d_depth), p(d_sem), N, T, t, Cn, float(c.density_scale)]
    tail = [p(G), p(d_h_c), p(d_h_f), p(pc), p(ps), ops._stream()]
    if x2:
        _lib.check(lib.ucsa_composite_bwd_x2(*head, *tail), "ucsa_composite_bwd_x2")
    elif half:
        _lib.check(lib.ucsa_composite_bwd_f16(*head, float(f16_scale), *tail), "ucsa_composite_bwd_f16")
    else:
        _lib.check(lib.ucsa_composite_bwd(*head, *tail), "ucsa_composite_bwd")
    torch.cuda.synchronize()
    for name, v in (("partial_color", pc), ("partial_sem", ps)):
        assert bool(torch.isfinite(v).all()), f"{name}: a wave left its slot unwritten"
    gc, gsem = torch.empty(7168, device="cuda"), torch.empty(ps.shape[1], device="cuda")
    ops.reduce_partials(pc, gc, False)
    ops.reduce_partials(ps, gsem, False)
    torch.cuda.synchronize()
    return dict(G=G, d_h_c=d_h_c, d_h_f=d_h_f, dW_color=gc, dW_sem=gsem)


BWD = {"composite_bwd": ("fp32", "fp32", 1.0), "composite_bwd_f16_scale1": ("f16(gs=1024)", "f16", 1.0),
       "composite_bwd_f16_scale1024": ("f16(gs=1024)", "f16", 1024.0),
       "composite_bwd_x2": ("bf16x2", "x2", 1.0)}


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("entry", list(BWD))
def test_backward(ops, entry, case):
    """Fed the reference's src and its fp32-rounded weights: G, d_h_c, d_h_f
    row by row, dW_color and dW_sem after reduce_partials.  _f16 against the
    fp16-emulating reference (gradients rounded under the same scale)."""
    pin, kind, gs = BWD[entry]
    c = _case(*case, pin)
    src, w32, ref = _ref_backward(*case, pin, kind, gs)
    got = _composite_bwd(ops, c, src, w32, kind, gs)
    sn.compare_backward(got, ref, f"{entry} {case[0]}", c.name)


SINGLE = [("blocks", None), ("classes", 17), ("classes", 61), ("long", (96, 34))]


@pytest.mark.parametrize("case", SINGLE, ids=case_id)
@pytest.mark.parametrize("entry", ["composite_bwd", "composite_bwd_f16_scale1024", "composite_bwd_x2"])
def test_single_kernel_backward(ops, entry, case):
    """UCSA_SHADE_BWD_SPLIT=0 + ucsa_env_reload() selects k_shade_bwd<NRB,
    false, H, NET = 0> inside this process: the fp32 and f16 backward again;
    _x2 exists as the per-net pair only and must return its argument-0 error,
    which is also what shows that the switch was followed."""
    from ucsa_neural_rendering_amd import _lib
    pin, kind, gs = BWD[entry]
    c = _case(*case, pin)
    src, w32, ref = _ref_backward(*case, pin, kind, gs)
    before = os.environ.get("UCSA_SHADE_BWD_SPLIT")
    os.environ["UCSA_SHADE_BWD_SPLIT"] = "0"
    try:
        ops.env_reload()
        assert not ops.shade_bwd_split()
        if kind == "x2":
            with pytest.raises(_lib.UcsaError, match=r"code -1000\b"):
                _composite_bwd(ops, c, src, w32, kind, gs)
        else:
            got = _composite_bwd(ops, c, src, w32, kind, gs)
            sn.compare_backward(got, ref, f"{entry} single-kernel {case[0]}", c.name)
    finally:
        if before is None:
            os.environ.pop("UCSA_SHADE_BWD_SPLIT", None)
        else:
            os.environ["UCSA_SHADE_BWD_SPLIT"] = before
        ops.env_reload()
    if ops.shade_bwd_split() and kind == "x2":
        # ... and back: the pair is selected again
        got = _composite_bwd(ops, c, src, w32, kind, gs)
        sn.compare_backward(got, ref, f"{entry} {case[0]}", c.name)


# ---------------------------------------------------------------------------
# sigma net
# ---------------------------------------------------------------------------
SIGMA = {"sigma_mlp_bwd": (sn.FP32, False), "sigma_mlp_bwd_h16": (sn.FP32, True),
         "sigma_mlp_bwd_x2": (sn.X2, False)}


@functools.lru_cache(maxsize=None)
def _sigma_case(M):
    return sn.build_sigma_case(_field(40).sigma_params.numpy(), M)


@pytest.mark.parametrize("M", sn.SIGMA_M)
@pytest.mark.parametrize("entry", list(SIGMA))
def test_sigma_backward(ops, entry, M):
    """d_feat and dW per element; a tenth of the d_h rows are zero, one feat
    row is (its gates sit at an exact zero: closed); partials pre-filled with NaN."""
    from ucsa_neural_rendering_amd import _lib
    lib = _lib.lib()
    mode, h16 = SIGMA[entry]
    c = _sigma_case(M)
    ref = sn.sigma_backward(c.feat, c.d_h, c.sigma_params, mode, h16)
    sp = _dev(c.sigma_params)
    x2 = entry.endswith("_x2")
    packed = (ops.mlp_pack_x3 if x2 else ops.mlp_pack)(_lib.MLP_SIGMA, sp)
    packed_t = (ops.mlp_pack_t_x3 if x2 else ops.mlp_pack_t)(_lib.MLP_SIGMA, sp)
    feat = _dev(c.feat).view(M, 16, 2).permute(1, 0, 2).contiguous()
    d_h = _dev(c.d_h)
    parts = int(lib.ucsa_sigma_mlp_bwd_parts(M))
    d_feat = torch.full((16, M, 2), float("nan"), device="cuda")
    partial = torch.full((parts, 3072), float("nan"), device="cuda")
    fn = getattr(lib, "ucsa_" + entry)
    p = ops._ptr
    _lib.check(fn(p(feat), p(d_h), p(packed), p(packed_t), M, 16, p(d_feat), p(partial), ops._stream()),
               "ucsa_" + entry)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(partial).all()), "a wave left its partial slot unwritten"
    gW = torch.empty(3072, device="cuda")
    ops.reduce_partials(partial, gW, False)
    torch.cuda.synchronize()
    sn.compare_sigma(dict(d_feat=d_feat.permute(1, 0, 2).reshape(M, 32), dW=gW), ref, entry, c.name)
