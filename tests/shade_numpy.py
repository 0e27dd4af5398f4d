"""numpy restatement of the colour / semantics / compositing stage and of its
backward (include/ucsa_hip.h: ``ucsa_composite_fwd*``, ``ucsa_composite_train_fwd_*``,
``ucsa_composite_bwd*``) and of the sigma net, backward (``ucsa_sigma_mlp_bwd*``)
and forward (``ucsa_sigma_mlp_fwd*``: ``sigma_forward(outputs=True)``, used
through tests/density_numpy.py):
the float64 yardstick of tests/test_shade_reference_cpu.py and
tests/test_gpu_shade_reference.py (test infrastructure: plain numpy, no torch
op, no GPU, no HIP library).

It is stated from ``oracle/renderer.py`` (``run``: merge, ``alpha_weights``, the
``w > 1e-4`` mask, the three sums) and ``oracle/field.py`` (``sh4_encode``,
the ``mlp_split`` layout, ``color``, ``semantics``, ``_TruncExp``), with the
backward written out by hand.  It knows nothing of waves, 16-blocks, pending
lists or per-wave partials: one row per sample, one sum per ray.

Every function that returns a value ``v`` also returns ``e_v``, a per-element
bound on |kernel - v| obtained by RUNNING ERROR ANALYSIS: each contraction
``y = sum_k x_k w_k`` of K terms contributes

    e_y = sum_k e_x_k |w_k|  +  ((K + 1) u + p) sum_k |x_k w_k|

(the inputs' own bounds pushed through, K fused multiply-adds of one rounding
each in ANY order, one rounding of slack, and the mode's unit per product p),
``u = 2^-24``.  The units per product are the ones the sources document:

* ``FP32``   f32-input MFMA chain: p = 0 (the fmaf roundings are the K u);
* ``X2``     two-term bf16 operands (mfma_mlp_x3.h "bf16x2"): p = 2^-16;
* ``X3``     three-term bf16 / two-term f16 FORWARDS (mfma_mlp_x3.h,
             mfma_mlp_h2.h): both operand splits keep 2^-23, what is dropped
             is <= 2^-23: p = 2^-21;
* ``H2``     the f16x2 forward besides: an operand below 2^-13 keeps an
             ABSOLUTE 2^-36 instead (mfma_mlp_h2.h): + 2^-36 (sum |x| + sum |w|);
* ``F16(gs)`` fp16 weights and layer inputs, quantisation EMULATED here (the
             reference rounds exactly where the kernel does, gradients under
             the loss scale ``gs`` included), products of two fp16 values are
             exact in fp32, so p = 0 -- but a value the kernel rounds to fp16
             differs from the reference's by its bound e, and where the
             reference's value lies within e of an fp16 rounding boundary the
             two may round apart: such an element carries ONE fp16 ulp
             instead of e (``_q``); everywhere else rounding REMOVES e.

``expf`` (libm, the weights): 1 ulp = 2^-23 relative.  ``__expf`` (hardware
exp2 of x log2e, composite_common.h "~2 ulp"): 2^-22 + |x| u.  Hardware
reciprocal: 1 ulp.

ReLU gates and the mask are NOT in the tolerance: the case builders at the end
redraw any sample whose hidden pre-activation lies within its own bound of
zero, or whose weight lies within its bound of 1e-4, until none is left (at
most 5 % of a case's samples, asserted), so the kernel and the reference take
the same branch everywhere and every comparison is element by element.

``dt=F32`` evaluates the same formulas in plain fp32 with sequential sums (for
the test that the bounds are not tighter than fp32 arithmetic allows);
``mutant`` names one deliberate mistake (for the sharpness tests).
"""
import math
from types import SimpleNamespace as NS

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
U = 2.0 ** -24                     # unit round-off of fp32
W_MIN = 1e-4                       # the mask threshold
TINY = 2.0 ** -149                 # smallest fp32 subnormal (expf flushes below)
LO, HI = math.exp(-15.0), math.exp(15.0)

MUTANTS = ("next_ray_dimage", "tail_shift", "gate_ge", "sem_not_detached",
           "drop_1e15", "last_delta_prev", "no_clamp", "suffix_inclusive",
           "carry_lost_64", "softmax_padded", "unstable_merge", "depth_no_norm")


def _np(a, dtype):
    if a is None:
        return None
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype))


class Mode:
    def __init__(self, name, prod=0.0, half=False, gs=1.0, round_grads=True, absop=0.0):
        self.name, self.prod, self.half, self.gs = name, float(prod), bool(half), float(gs)
        self.absop = float(absop)           # absolute error of one operand (f16x2 below 2^-13)
        self.round_grads = round_grads      # False: gradients pass unrounded (the oracle's
                                            # straight-through fp16 emulation)

    def __repr__(self):
        return self.name


FP32 = Mode("fp32")
X2 = Mode("bf16x2", prod=2.0 ** -16)
X3 = Mode("x3", prod=2.0 ** -21)
H2 = Mode("h2", prod=2.0 ** -21, absop=2.0 ** -36)


def F16M(gs=1024.0, round_grads=True):
    return Mode(f"f16(gs={gs:g})", half=True, gs=gs, round_grads=round_grads)


# ---------------------------------------------------------------------------
# fp16 quantisation with its boundary bound
# ---------------------------------------------------------------------------
def q16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, F64).astype(F16).astype(F64)


def _q(v, e, mode, scale=None):
    """What an fp16 MFMA operand holds: ``f16(v * scale) / scale``.  The kernel
    rounds ITS fp32 value, within e of v.  Both round to the same fp16 number
    unless a rounding boundary lies within e * scale of v * scale: then they
    may differ by one fp16 ulp.  Boundaries sit half an ulp from q (a quarter
    below a power of two: both are tested).  Outside fp16 mode: (v, e)."""
    if not mode.half or (scale is not None and not mode.round_grads):
        return v, e
    scale = 1.0 if scale is None else scale
    x = np.asarray(v, F64) * scale
    q = q16(x)
    ulp = np.spacing(np.abs(q).astype(F16)).astype(F64)
    r = np.abs(x - q)
    near = np.minimum(np.abs(r - 0.5 * ulp), np.abs(r - 0.25 * ulp)) <= np.asarray(e, F64) * scale
    return q / scale, np.where(near, ulp, 0.0) / scale


# ---------------------------------------------------------------------------
# contractions
# ---------------------------------------------------------------------------
def _dot(x, W, dt):
    """x [n, K] . W [O, K]^T.  fp32: one product and one addition per term,
    sequentially in k (nothing like the MFMA chain's order)."""
    if dt is F64:
        return x @ W.T
    acc = np.zeros((x.shape[0], W.shape[0]), dt)
    for k in range(W.shape[1]):
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    return acc


def _lin(x, ex, W, mode, dt):
    """-> (x W^T, its bound): see the module docstring."""
    y = _dot(x, W, dt)
    x64, W64 = np.abs(np.asarray(x, F64)), np.abs(np.asarray(W, F64))
    K = W.shape[1]
    ey = np.asarray(ex, F64) @ W64.T + ((K + 1) * U + mode.prod) * (x64 @ W64.T)
    if mode.absop:
        ey = ey + mode.absop * (x64.sum(1, keepdims=True) + W64.sum(1)[None, :])
    return y, ey


def _outer(dy, edy, x, ex, mode, dt, n_terms):
    """dW = dy^T x over the samples, summed in ANY order (16 at a time in a
    wave's accumulators, waves reduced afterwards): the factors' bounds pushed
    through, (n + 3) u for the additions and the product, the mode's unit."""
    if dt is F64:
        dW = dy.T @ x
    else:
        dW = np.zeros((dy.shape[1], x.shape[1]), dt)
        for i in range(dy.shape[0]):
            dW = dW + dy[i][:, None] * x[i][None, :]
    a, b = np.abs(np.asarray(dy, F64)), np.abs(np.asarray(x, F64))
    e = edy.T @ b + a.T @ ex + ((n_terms + 3) * U + mode.prod) * (a.T @ b)
    return dW, e


# ---------------------------------------------------------------------------
# nets: tcnn-format flat parameters, row-major [out, in], padded shapes
# ---------------------------------------------------------------------------
def split_nets(color_params, sem_params, C, mode=FP32, dt=F64):
    nrb = (C + 15) // 16
    c, s = _np(color_params, F64), _np(sem_params, F64)
    assert c.size == 7168 and s.size == 1024 + 1024 * nrb
    if mode.half:
        c, s = q16(c), q16(s)
    c, s = c.astype(dt), s.astype(dt)
    return NS(c1=c[:2048].reshape(64, 32), c2=c[2048:6144].reshape(64, 64),
              c3=c[6144:].reshape(16, 64), s1=s[:1024].reshape(64, 16),
              s2=s[1024:].reshape(16 * nrb, 64), nrb=nrb)


_SH = (0.28209479177387814, 0.48860251190291987, 1.0925484305920792,
       0.94617469575755997, 0.31539156525251999, 0.54627421529603959,
       0.59004358992664352, 2.8906114426405538, 0.45704579946446572,
       0.3731763325901154, 1.4453057213202769)


def _sh_terms(x, y, z, s):
    """oracle.field.sh4_encode; s = -1 as written, s = +1 with every
    subtraction turned into an addition (for |x|, |y|, |z|: the sum of the
    absolute values of the monomials)."""
    k = [x.dtype.type(v) for v in _SH]
    n = x.dtype.type(s)
    xy, xz, yz = x * y, x * z, y * z
    x2, y2, z2 = x * x, y * y, z * z
    three, five, one = x.dtype.type(3.0), x.dtype.type(5.0), x.dtype.type(1.0)
    return np.stack([
        np.full_like(x, k[0]), n * k[1] * y, k[1] * z, n * k[1] * x,
        k[2] * xy, n * k[2] * yz, k[3] * z2 + n * k[4], n * k[2] * xz,
        k[5] * x2 + n * k[5] * y2,
        k[6] * y * (n * three * x2 + y2),
        k[7] * xy * z,
        k[8] * y * (one + n * five * z2),
        k[9] * z * (five * z2 + n * three),
        k[8] * x * (one + n * five * z2),
        k[10] * z * (x2 + n * y2),
        k[6] * x * (n * x2 + three * y2)], axis=-1)


def sh4(dirs, dt=F64):
    """Degree-4 spherical harmonics of (d + 1) / 2 as tcnn maps it back
    (2 d01 - 1).  Bound: the kernel's coordinate carries <= 2 u (the rounding of
    d + 1 <= 2; / 2, * 2 and - 1 are exact), each harmonic <= 6 operations.
    With P the harmonic's polynomial with absolute monomials -- monotone in
    |x|, |y|, |z| -- |sh(x~) - sh(x)| <= P(|x| + 2u) - P(|x|), plus 6 u P."""
    d = np.asarray(dirs, dt)
    d01 = (d + dt(1.0)) / dt(2.0)
    c = d01 * dt(2.0) - dt(1.0)
    sh = _sh_terms(c[:, 0], c[:, 1], c[:, 2], -1.0)
    a = np.abs(np.asarray(dirs, F64))
    p0 = np.abs(_sh_terms(a[:, 0], a[:, 1], a[:, 2], 1.0))
    a = a + 2.0 * U
    p1 = np.abs(_sh_terms(a[:, 0], a[:, 1], a[:, 2], 1.0))
    e = (p1 - p0) + 6.0 * U * p1
    e[:, 0] = 0.0
    return sh, e


def _exp_rel(x):
    """hardware exponential of x: exp2(x * log2e).  2^-22 (composite_common.h:
    "~2 ulp") plus the rounding of the product in the exponent, |x| u."""
    return 2.0 ** -22 + np.abs(np.asarray(x, F64)) * U


def _relu_e(a, e):
    """bound of relu(a): a unit that is off is exactly 0 on both sides.  (Valid
    because no pre-activation of an accepted input lies within its bound of
    zero; a row where one does is redrawn whatever its later layers say.)"""
    return np.where(np.asarray(a, F64) > 0, e, 0.0)


def shade_forward(dirs, geo, nets, C, mode=FP32, dt=F64, mutant=()):
    """The two nets on n samples: dirs [n, 3], geo [n, 15] -> every
    pre-activation, layer input, rgb [n, 3], p [n, C] and their bounds.
    colour input = [sh16 | geo15 | 1], semantics input = [geo15 | 1] (the input
    padded to a multiple of 16 with the constant 1.0)."""
    assert dt is F64 or not mode.half
    n = dirs.shape[0]
    geo = np.asarray(geo, dt).reshape(n, 15)
    one = np.ones((n, 1), dt)
    sh, e_sh = sh4(dirs, dt)
    f = NS(n=n)
    x1 = np.concatenate([sh, geo, one], 1)
    e_x1 = np.concatenate([e_sh, np.zeros((n, 16))], 1)
    f.x1, f.e_x1 = _q(x1, e_x1, mode)
    f.a1, f.e_a1 = _lin(f.x1, f.e_x1, nets.c1, mode, dt)
    f.h1, f.e_h1 = _q(np.maximum(f.a1, 0), _relu_e(f.a1, f.e_a1), mode)
    f.a2, f.e_a2 = _lin(f.h1, f.e_h1, nets.c2, mode, dt)
    f.h2, f.e_h2 = _q(np.maximum(f.a2, 0), _relu_e(f.a2, f.e_a2), mode)
    o3, e_o3 = _lin(f.h2, f.e_h2, nets.c3, mode, dt)
    f.o3, f.e_o3 = o3[:, :3], e_o3[:, :3]
    # sigmoid = rcp(1 + exp(-o)): d/do = s (1 - s); the exponential's relative
    # error enters through the same derivative; the addition and the
    # reciprocal are one ulp each of s
    f.rgb = dt(1.0) / (dt(1.0) + np.exp(-f.o3))
    s = np.asarray(f.rgb, F64)
    f.e_rgb = s * (1.0 - s) * (f.e_o3 + _exp_rel(f.o3)) + 4.0 * U * s
    # semantics
    xs = np.concatenate([geo, one], 1)
    f.xs, f.e_xs = _q(xs, np.zeros((n, 16)), mode)
    f.a1s, f.e_a1s = _lin(f.xs, f.e_xs, nets.s1, mode, dt)
    f.hs, f.e_hs = _q(np.maximum(f.a1s, 0), _relu_e(f.a1s, f.e_a1s), mode)
    f.lg, f.e_lg = _lin(f.hs, f.e_hs, nets.s2, mode, dt)
    Cs = nets.s2.shape[0] if "softmax_padded" in mutant else C
    l = f.lg[:, :Cs]
    m = l.max(1, keepdims=True) if n else l[:, :1]
    ex = np.exp(l - m)
    p = ex / ex.sum(1, keepdims=True)
    # p_c = E_c / sum E: E_c carries e_l_c + e_max (<= 2 max e_l) and the
    # exponential's own error, the sum no more than its worst term plus C
    # additions, the reciprocal and the product one ulp each
    rng = np.abs(np.asarray(l - m, F64)).max(1, keepdims=True) if n else np.zeros((0, 1))
    e_l = f.e_lg[:, :Cs].max(1, keepdims=True) if n else np.zeros((0, 1))
    rel = 2.0 * (2.0 * e_l + _exp_rel(rng) + U) + (Cs + 4) * U
    f.p = np.zeros((n, nets.s2.shape[0]), dt)
    f.p[:, :Cs] = p
    f.e_p = np.asarray(f.p, F64) * rel
    f.C = Cs
    return f


def _gate(pre, mutant):
    return (pre >= 0) if "gate_ge" in mutant else (pre > 0)


def shade_backward(f, w, di, dd, ds, zz, nrm, nets, C, mode=FP32, dt=F64, mutant=()):
    """Backward of ``shade_forward`` for n masked samples carrying weight w [n],
    their ray's d_image di [n, 3], d_depth dd [n], d_semantics ds [n, C], norm
    nrm [n] and their depth zz [n].
      G     = d_depth z / norm + d_image . rgb     (colour / depth path only:
              the semantic weights are detached)
      d_geo = W1c^T(geo rows) d_hid1 + W1s^T d_hid_s
      dW    = sum over the samples of d_out (x) layer input
    In fp16 mode every gradient vector is rounded once to fp16 under the loss
    scale before its two uses (dX and dW), as chain_h / dw_accumulate_h do."""
    n = f.n
    one = dt(1.0)
    w, dd, zz, nrm = (np.asarray(v, dt).reshape(n) for v in (w, dd, zz, nrm))
    di = np.asarray(di, dt).reshape(n, 3)
    ds = np.asarray(ds, dt).reshape(n, C)
    gs = mode.gs
    b = NS()
    rgb, e_rgb = f.rgb, f.e_rgb
    a64 = lambda v: np.abs(np.asarray(v, F64))
    # G: one product and one division for the depth term, three products and
    # three additions
    g0 = dd * zz / nrm
    b.G = g0 + (di * rgb).sum(1)
    A_G = a64(g0) + (a64(di) * a64(rgb)).sum(1)
    b.e_G = (a64(di) * e_rgb).sum(1) + 8.0 * U * A_G
    if "sem_not_detached" in mutant:
        b.G = b.G + (ds * f.p[:, :C]).sum(1)
    # d_o3 = w d_image rgb (1 - rgb): d/d rgb = 1 - 2 rgb; four roundings
    dy3 = np.zeros((n, 16), dt)
    dy3[:, :3] = w[:, None] * di * rgb * (one - rgb)
    e_dy3 = np.zeros((n, 16))
    e_dy3[:, :3] = (a64(w)[:, None] * a64(di) * a64(one - 2 * rgb) * e_rgb
                    + 5.0 * U * a64(dy3[:, :3]))
    dy3, e_dy3 = _q(dy3, e_dy3, mode, gs)
    nt = n
    b.dWc3, b.e_dWc3 = _outer(dy3, e_dy3, f.h2, f.e_h2, mode, dt, nt)
    dh2, e = _lin(dy3, e_dy3, nets.c3.T, mode, dt)
    g2 = _gate(f.a2, mutant)
    dh2, e = _q(np.where(g2, dh2, 0), np.where(g2, e, 0.0), mode, gs)
    b.dWc2, b.e_dWc2 = _outer(dh2, e, f.h1, f.e_h1, mode, dt, nt)
    dh1, e = _lin(dh2, e, nets.c2.T, mode, dt)
    g1 = _gate(f.a1, mutant)
    dh1, e = _q(np.where(g1, dh1, 0), np.where(g1, e, 0.0), mode, gs)
    b.dWc1, b.e_dWc1 = _outer(dh1, e, f.x1, f.e_x1, mode, dt, nt)
    dx1, e_dx1 = _lin(dh1, e, nets.c1.T, mode, dt)
    dgeo_c, e_c = dx1[:, 16:31], e_dx1[:, 16:31]
    # semantics = sum w_detached p: d_p = w d_sem; softmax backward
    # d_l = p (d_p - p . d_p)
    Cs = f.C
    dp = np.zeros((n, nets.s2.shape[0]), dt)
    dp[:, :C] = w[:, None] * ds
    e_dp = U * a64(dp)
    p, e_p = f.p, f.e_p
    dot = (p * dp).sum(1, keepdims=True)
    A_dot = (a64(p) * a64(dp)).sum(1, keepdims=True)
    e_dot = (e_p * a64(dp) + a64(p) * e_dp).sum(1, keepdims=True) + (Cs + 2) * U * A_dot
    diff = dp - dot
    dlg = p * diff
    e_dlg = e_p * a64(diff) + a64(p) * (e_dp + e_dot + U * a64(diff)) + 2.0 * U * a64(dlg)
    dlg[:, Cs:] = 0
    e_dlg[:, Cs:] = 0.0
    dlg, e_dlg = _q(dlg, e_dlg, mode, gs)
    b.dWs2, b.e_dWs2 = _outer(dlg, e_dlg, f.hs, f.e_hs, mode, dt, nt)
    dhs, e = _lin(dlg, e_dlg, nets.s2.T, mode, dt)
    gsm = _gate(f.a1s, mutant)
    dhs, e = _q(np.where(gsm, dhs, 0), np.where(gsm, e, 0.0), mode, gs)
    b.dWs1, b.e_dWs1 = _outer(dhs, e, f.xs, f.e_xs, mode, dt, nt)
    dxs, e_dxs = _lin(dhs, e, nets.s1.T, mode, dt)
    dgeo_s, e_s = dxs[:, :15], e_dxs[:, :15]
    # the two parts meet in one addition (and one multiplication by 1 / gs, a
    # power of two)
    b.dgeo = dgeo_c + dgeo_s
    b.e_dgeo = e_c + e_s + U * (a64(dgeo_c) + a64(dgeo_s))
    b.dW_color = np.concatenate([b.dWc1.ravel(), b.dWc2.ravel(), b.dWc3.ravel()])
    b.e_dW_color = np.concatenate([b.e_dWc1.ravel(), b.e_dWc2.ravel(), b.e_dWc3.ravel()])
    b.dW_sem = np.concatenate([b.dWs1.ravel(), b.dWs2.ravel()])
    b.e_dW_sem = np.concatenate([b.e_dWs1.ravel(), b.e_dWs2.ravel()])
    return b


# ---------------------------------------------------------------------------
# merge and weights
# ---------------------------------------------------------------------------
def merge_src(z_c, z_f, mutant=()):
    """src [N, S]: the stable ascending sort of [coarse | fine] (torch.sort of
    the concatenation: on ties the lower index, so coarse before fine)."""
    z = _np(z_c, F32) if z_f is None else np.concatenate([_np(z_c, F32), _np(z_f, F32)], 1)
    if "unstable_merge" in mutant:
        idx = np.arange(z.shape[1])
        return np.stack([np.lexsort((-idx, row)) for row in z]).astype(np.int32)
    return np.argsort(z, axis=1, kind="stable").astype(np.int32)


def ray_weights(zs, sg, density_scale, dt=F64, mutant=()):
    """oracle.renderer.alpha_weights on sorted depths zs [N, S], sigmas sg:
    delta (last 1e10), ex = exp(-delta scale sigma), alpha = 1 - ex,
    fac = 1 - alpha + 1e-15, T = exclusive product of fac, w = alpha T.
    Bounds, absolute (an opaque sample makes fac = 1e-15, relative errors mean
    nothing there):
      x = delta scale sigma: the subtraction and two products, 3 u x
      ex: expf, 1 ulp = 2 u, plus the argument's error, plus flush to zero
      alpha: + u alpha;   fac: + 2 u fac
      T_{i+1} = T_i fac_i: e_T fac + T e_fac + u T_{i+1}; the kernel's scan is
      a tree (6 levels and one carry per 64-sample pass): + 8 u T for its shape
      w: e_alpha T + alpha e_T + u w"""
    zs, sg = np.asarray(zs, dt), np.asarray(sg, dt)
    N, S = zs.shape
    delta = np.empty_like(zs)
    delta[:, :-1] = zs[:, 1:] - zs[:, :-1]
    delta[:, -1] = dt(1e10)
    if "last_delta_prev" in mutant and S > 1:
        delta[:, -1] = delta[:, -2]
    x = delta * dt(density_scale) * sg
    with np.errstate(under="ignore"):
        ex = np.exp(-x)
    alpha = dt(1.0) - ex
    fac = dt(1.0) - alpha if "drop_1e15" in mutant else dt(1.0) - alpha + dt(1e-15)
    T = np.ones_like(zs)
    for i in range(1, S):
        T[:, i] = T[:, i - 1] * fac[:, i - 1]
        if "carry_lost_64" in mutant and i % 64 == 0:
            T[:, i] = 1.0
    w = alpha * T
    x64, ex64, al64, fac64, T64 = (np.asarray(v, F64) for v in (x, ex, alpha, fac, T))
    e_ex = ex64 * (3.0 * U * np.abs(x64) + 2.0 * U) + TINY
    e_alpha = e_ex + U * np.abs(al64)
    e_fac = e_alpha + 2.0 * U * fac64
    e_T = np.zeros((N, S))
    for i in range(1, S):
        e_T[:, i] = e_T[:, i - 1] * fac64[:, i - 1] + T64[:, i - 1] * e_fac[:, i - 1] + U * T64[:, i]
    e_T = e_T + 8.0 * U * T64
    e_w = e_alpha * T64 + np.abs(al64) * e_T + U * np.abs(np.asarray(w, F64))
    return NS(delta=delta, ex=ex, alpha=alpha, fac=fac, T=T, w=w, e_ex=e_ex,
              e_fac=e_fac, e_T=e_T, e_w=e_w)


def _gather_sorted(src, T, a_c, a_f, dt):
    a = _np(a_c, dt) if a_f is None else np.concatenate([_np(a_c, dt), _np(a_f, dt)], 1)
    return np.take_along_axis(a, src.astype(np.int64), 1)


def _rows(h_c, h_f, N, T, t):
    hc = _np(h_c, F32).reshape(N, T, 16)
    if t == 0:
        return hc
    return np.concatenate([hc, _np(h_f, F32).reshape(N, t, 16)], 1)


def _shade_rows(rays_d, h_all, src, mask, mutant):
    """(ray, sorted slot) of every masked sample and the h row it is shaded with."""
    ray, slot = np.nonzero(mask)
    use = slot.copy()
    if "tail_shift" in mutant:
        S = mask.shape[1]
        cnt = mask.sum(1)
        rank = np.cumsum(mask, 1)[ray, slot] - 1
        tail = rank >= (cnt[ray] // 16) * 16
        use = np.where(tail, np.minimum(slot + 1, S - 1), slot)
    rows = h_all[ray, src[ray, use]]
    return ray, slot, rows


def composite_forward(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                      color_params, sem_params, C, density_scale, mode=FP32,
                      dt=F64, mutant=()):
    """oracle.renderer.run from the merge on.  -> src, weights, mask, image,
    depth = sum(w z) / norm, semantics (softmax over the C real classes, masked
    rows only) and their bounds.  The three sums run over the masked samples in
    any order: (n + 2) u of the sum of absolute terms."""
    rays_d, norms = _np(rays_d, F32).reshape(-1, 3), _np(norms, F32).reshape(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    S = T + t
    r = NS(N=N, T=T, t=t, S=S, C=C)
    r.src = merge_src(z_c, z_f, mutant)
    r.zs = _gather_sorted(r.src, T, z_c, z_f, dt)
    r.sg = _gather_sorted(r.src, T, sigma_c, sigma_f, dt)
    r.rw = ray_weights(r.zs, r.sg, density_scale, dt, mutant)
    r.weights, r.e_weights = r.rw.w, r.rw.e_w
    r.mask = r.weights > dt(W_MIN)
    nets = split_nets(color_params, sem_params, C, mode, dt)
    ray, slot, rows = _shade_rows(rays_d, _rows(h_c, h_f, N, T, t), r.src, r.mask, mutant)
    f = shade_forward(rays_d[ray], rows[:, 1:], nets, C, mode, dt, mutant)
    w = r.weights[ray, slot]
    w64, e_w = np.asarray(w, F64), r.e_weights[ray, slot]
    n_ray = r.mask.sum(1)

    def ray_sum(val, e_val, extra=0.0):
        """sum_s w val over each ray's masked samples, with its bound."""
        term = w[:, None] * val
        out = np.zeros((N, val.shape[1]), dt)
        np.add.at(out, ray, term)
        A = np.zeros((N, val.shape[1]))
        E = np.zeros((N, val.shape[1]))
        np.add.at(A, ray, np.abs(np.asarray(term, F64)))
        np.add.at(E, ray, e_w[:, None] * np.abs(np.asarray(val, F64)) + w64[:, None] * e_val)
        return out, E + ((n_ray[:, None] + 2) * U + extra) * A

    r.image, r.e_image = ray_sum(f.rgb, f.e_rgb)
    r.semantics, r.e_semantics = ray_sum(f.p[:, :C], f.e_p[:, :C])
    d, e_d = ray_sum(r.zs[ray, slot][:, None], np.zeros((len(ray), 1)), U)
    if "depth_no_norm" in mutant:
        r.depth, r.e_depth = d[:, 0], e_d[:, 0]
    else:
        r.depth = d[:, 0] / norms.astype(dt)
        r.e_depth = e_d[:, 0] / norms.astype(F64) + U * np.abs(np.asarray(r.depth, F64))
    r.f, r.ray, r.slot = f, ray, slot
    return r


def weights_backward(G, e_G, w32, zs, sg, density_scale, dt=F64, mutant=()):
    """d h0 of every sample from G [N, S] (zero outside the mask):
      d_alpha_i = G_i T_i - (sum_{j > i} G_j w_j) / (1 - alpha_i + 1e-15)
      d_sigma_i = d_alpha_i ex_i delta_i scale
      d_h0_i    = d_sigma_i clamp(sigma_i, e^-15, e^15)      (_TruncExp)
    with w the fp32 weights the entry point receives and T, ex, delta
    recomputed from the depths and sigmas (``ray_weights``).
    Bounds: the suffix sum is a scan (6 levels, one carry per pass, one product
    per term): (S / 64 + 8) u of the absolute sum, plus e_G w; the quotient
    e_suf / fac + |suf| e_fac / (fac (fac - e_fac)) -- infinite when fac is not
    told from zero, which costs nothing where ex is exactly 0 on both sides
    (the product is then exactly 0); three roundings for ex delta scale, one
    per product after it, and the clamp ends e^(+-15) as fp32 numbers."""
    N, S = G.shape
    G, w = np.asarray(G, dt), np.asarray(w32, dt)
    rw = ray_weights(zs, sg, density_scale, dt, mutant)
    a64 = lambda v: np.abs(np.asarray(v, F64))
    q = G * w
    rev = np.cumsum(q[:, ::-1], 1)[:, ::-1]
    A_rev = np.cumsum(a64(q)[:, ::-1], 1)[:, ::-1]
    E_rev = np.cumsum((np.asarray(e_G, F64) * a64(w))[:, ::-1], 1)[:, ::-1]
    if "suffix_inclusive" in mutant:
        suf, A_suf, E_suf = rev, A_rev, E_rev
    else:
        z1 = np.zeros((N, 1))
        suf = np.concatenate([rev[:, 1:], z1.astype(dt)], 1)
        A_suf = np.concatenate([A_rev[:, 1:], z1], 1)
        E_suf = np.concatenate([E_rev[:, 1:], z1], 1)
    if "carry_lost_64" in mutant:
        # the reverse scan runs in passes of 64 from the far end: a pass that
        # forgets the carry sees only its own samples
        k = S - 1 - np.arange(S)
        first = S - (k // 64) * 64                 # where the passes before this one begin
        suf = suf - np.concatenate([rev, np.zeros((N, 1), dt)], 1)[:, first]
    e_suf = E_suf + (S / 64.0 + 8.0) * U * A_suf
    fac64, T64 = np.asarray(rw.fac, F64), np.asarray(rw.T, F64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        quo = suf / rw.fac
        lo = fac64 - rw.e_fac
        e_quo = np.where(lo > 0, e_suf / fac64 + a64(suf) * rw.e_fac / (fac64 * lo), np.inf)
        e_quo = np.where((a64(suf) == 0) & (e_suf == 0), 0.0, e_quo)
        t1 = G * rw.T
        da = t1 - quo
        e_da = (np.asarray(e_G, F64) * T64 + a64(G) * rw.e_T + U * a64(t1) + e_quo
                + U * a64(quo) + U * a64(da))
        m = rw.ex * rw.delta * dt(density_scale)
        m64 = np.asarray(m, F64)
        e_m = rw.e_ex * a64(rw.delta) * density_scale + 3.0 * U * m64
        dsig = da * m
        e_dsig = np.where(m64 == 0, 0.0, e_da * m64) + np.where(np.isfinite(a64(da)), a64(da), np.inf) * e_m \
            + U * a64(dsig)
        c = np.asarray(sg, dt) if "no_clamp" in mutant else np.clip(np.asarray(sg, dt), dt(LO), dt(HI))
        dh0 = dsig * c
        e_dh0 = e_dsig * a64(c) + 3.0 * U * a64(dh0)
    return dh0, e_dh0


def composite_backward(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                       color_params, sem_params, C, density_scale, src, weights,
                       d_image, d_depth, d_sem, mode=FP32, dt=F64, mutant=()):
    """Backward of ``composite_forward`` wrt the h rows and both nets' weights,
    by hand.  ``src`` / ``weights`` are the int32 / fp32 arrays the entry point
    receives; the mask is ``weights > 1e-4f`` on those fp32 numbers, exactly as
    the kernel decides it.  -> G [N, S], d_h_c [N*T, 16], d_h_f [N*t, 16] | None,
    dW_color [7168], dW_sem, each with its bound e_*."""
    rays_d, norms = _np(rays_d, F32).reshape(-1, 3), _np(norms, F32).reshape(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    S = T + t
    src = _np(src, np.int32).reshape(N, S)
    w32 = np.asarray(_np(weights, None)).reshape(N, S)      # fp32 from the tests; kept as given
    d_image, d_depth = _np(d_image, F32).reshape(N, 3), _np(d_depth, F32).reshape(N)
    d_sem = _np(d_sem, F32).reshape(N, C)
    mask = w32 > F32(W_MIN)
    zs = _gather_sorted(src, T, z_c, z_f, dt)
    sg = _gather_sorted(src, T, sigma_c, sigma_f, dt)
    nets = split_nets(color_params, sem_params, C, mode, dt)
    ray, slot, rows = _shade_rows(rays_d, _rows(h_c, h_f, N, T, t), src, mask, mutant)
    f = shade_forward(rays_d[ray], rows[:, 1:], nets, C, mode, dt, mutant)
    up = ray.copy()
    if "next_ray_dimage" in mutant and len(ray):
        last = np.r_[ray[1:] != ray[:-1], True]
        up = np.where(last & (ray + 1 < N), ray + 1, ray)
    b = shade_backward(f, w32[ray, slot], d_image[up], d_depth[ray], d_sem[ray],
                       zs[ray, slot], norms[ray], nets, C, mode, dt, mutant)
    r = NS(mask=mask, f=f, b=b, ray=ray, slot=slot)
    r.G, r.e_G = np.zeros((N, S), dt), np.zeros((N, S))
    r.G[ray, slot], r.e_G[ray, slot] = b.G, b.e_G
    dh0, e_dh0 = weights_backward(r.G, r.e_G, w32, zs, sg, density_scale, dt, mutant)
    d_h, e_d_h = np.zeros((N, S, 16), dt), np.zeros((N, S, 16))
    rr = np.arange(N)[:, None].repeat(S, 1)
    d_h[rr, src, 0], e_d_h[rr, src, 0] = dh0, e_dh0
    e_src = src[ray, slot]
    d_h[ray, e_src, 1:], e_d_h[ray, e_src, 1:] = b.dgeo, b.e_dgeo
    r.d_h_c, r.e_d_h_c = d_h[:, :T].reshape(N * T, 16), e_d_h[:, :T].reshape(N * T, 16)
    r.d_h_f = r.e_d_h_f = None
    if t:
        r.d_h_f, r.e_d_h_f = d_h[:, T:].reshape(N * t, 16), e_d_h[:, T:].reshape(N * t, 16)
    r.dW_color, r.e_dW_color = b.dW_color, b.e_dW_color
    r.dW_sem, r.e_dW_sem = b.dW_sem, b.e_dW_sem
    return r


# ---------------------------------------------------------------------------
# sigma net: 32 -> 64 (ReLU) -> 16, no padding constant
# ---------------------------------------------------------------------------
H2_SIGMA_SCALE = 16.0              # ucsa_mlp_pack_h2: W1 x 2^-4, W2 x 2^4 (mfma_mlp_h2.h "RANGE")


def _q_hidden(v, e):
    """fp16 rounding of a layer input whose bound e need NOT be small against
    an fp16 ulp (a ReLU output next to zero sits among the fp16 subnormals):
    rounding is monotone, so the kernel's f16(v~), v~ in [v - e, v + e], lies in
    [f16(v - e), f16(v + e)].  The value is ``_q``'s; the bound is the larger of
    ``_q``'s and that interval's ends (they agree wherever e is below a
    quarter ulp)."""
    with np.errstate(invalid="ignore", over="ignore"):
        q, eq = _q(v, e, F16M(1.0))
        e = np.asarray(e, F64)
        span = np.maximum(np.abs(q16(v + e) - q), np.abs(q16(v - e) - q))
    return q, np.maximum(np.nan_to_num(eq, nan=0.0, posinf=np.inf), span)


F16_MIN = 2.0 ** -14               # smallest normal fp16


def _f16_subnormal_floor(x, W):
    """What an fp16 MFMA contraction x W^T of K terms may lose when an operand
    is an fp16 SUBNORMAL.  The matrix unit adds the K exact products as
    fixed-point numbers aligned to the largest product EXPONENT of the block
    and cuts them at fp32's 24 bits; a subnormal operand enters with the
    exponent of the smallest normal, 2^-14, however many leading zeros its
    mantissa has, so the cut lies up to 2^10 times higher above such a term
    than ``_lin``'s relative (K + 1) u allows for.  Charged: one cut (2^-23) of
    the largest NOMINAL product, max(|x|, 2^-14) max(|w|, 2^-14), per term,
    wherever a term has a non-zero subnormal operand; nothing elsewhere (an
    exact zero has no exponent to raise, normal operands are ``_lin``'s)."""
    x64, W64 = np.abs(np.asarray(x, F64)), np.abs(np.asarray(W, F64))
    sx, sw = (x64 > 0) & (x64 < F16_MIN), (W64 > 0) & (W64 < F16_MIN)
    nx, nw = np.where(sx, F16_MIN, x64), np.where(sw, F16_MIN, W64)
    with np.errstate(invalid="ignore"):
        worst = (nx * sx).max(1)[:, None] * nw.max(1)[None, :] + \
            np.where(np.isfinite(nx), nx, 0.0).max(1)[:, None] * (nw * sw).max(1)[None, :]
    return W.shape[1] * 2.0 ** -23 * worst


def sigma_forward(feat, sigma_params, mode=FP32, round_hidden=False, dt=F64,
                  e_feat=None, outputs=False):
    """The sigma net's first layer (what ``sigma_backward`` reads).

    ``outputs=True`` goes on to what ``ucsa_sigma_mlp_fwd*`` return: ``h``
    [M, 16], its bound ``e_h`` and ``sigma = exp(h[:, 0])`` as the allowed
    interval [``sigma_lo``, ``sigma_hi``] (``sigma_interval``).  Then, in fp16
    mode, the weights and the features are rounded to fp16 as the kernel loads
    them and the hidden activation is rounded after the ReLU (chain_relu_h);
    ``e_feat`` is the bound the features already carry (a hash-grid encode in
    front: the features are then taken as float64, not as fp32 inputs).

    Unlike the backward, the forward needs NO pinned gates: ReLU is
    1-Lipschitz, so a pre-activation within its bound e of zero gives an
    activation within e of the reference's whichever side either lies on;
    ``_relu_e`` holds everywhere else.

    f16x2 stores W1 x 2^-4 and W2 x 2^4 (``H2_SIGMA_SCALE``), so the ABSOLUTE
    2^-36 of an operand stored 16 times smaller -- a small W1 entry, a hidden
    activation -- counts 16 times against its partner: 15 ``absop`` sum |x| more
    on the first layer, 15 ``absop`` sum |W2| more on the second than ``_lin``
    charges for unscaled operands.

    fp16 mode: features below 2^-14 and hidden activations below 2^-14 are
    fp16 subnormals; both layers carry ``_f16_subnormal_floor``."""
    p = _np(sigma_params, F64)
    if outputs and mode.half:
        p = q16(p)
    p = p.astype(dt)
    W1, W2 = p[:2048].reshape(64, 32), p[2048:3072].reshape(16, 64)
    if e_feat is None:
        x = np.asarray(_np(feat, F32), dt).reshape(-1, 32)
        e_x = np.zeros(x.shape)
    else:
        x = np.asarray(feat, dt).reshape(-1, 32)
        e_x = np.asarray(e_feat, F64).reshape(-1, 32)
    if outputs:
        with np.errstate(invalid="ignore", over="ignore"):
            x, e_x = _q(x, e_x, mode)
            e_x = np.nan_to_num(e_x, nan=0.0, posinf=np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        a1, e_a1 = _lin(x, e_x, W1, mode, dt)
    if round_hidden:
        a1, e_a1 = _q(a1, e_a1, F16M(1.0))
    f = NS(W1=W1, W2=W2, x=x, a1=a1, e_a1=e_a1)
    if not outputs:
        return f
    x64, a64 = np.abs(np.asarray(x, F64)), np.asarray(a1, F64)
    extra = (H2_SIGMA_SCALE - 1.0) * mode.absop
    with np.errstate(invalid="ignore", over="ignore"):
        e_a1 = e_a1 + extra * x64.sum(1, keepdims=True)
        if mode.half:
            e_a1 = e_a1 + _f16_subnormal_floor(x, W1)
        f.e_a1 = e_a1
        hid = np.maximum(a1, 0)
        e_hid = np.where(np.abs(a64) <= e_a1, e_a1, _relu_e(a1, e_a1))
        if mode.half:
            hid, e_hid = _q_hidden(hid, e_hid)
        f.hid, f.e_hid = hid, e_hid
        f.h, e_h = _lin(hid, e_hid, W2, mode, dt)
        e_h = e_h + extra * np.abs(np.asarray(W2, F64)).sum(1)[None, :]
        if mode.half:
            e_h = e_h + _f16_subnormal_floor(hid, W2)
        # an all-zero input row is exact in every mode (the terms of a split 0
        # are 0, every product and sum is 0): no bound, absolute ones included
        zero = ((x64 == 0) & (e_x == 0)).all(1, keepdims=True)
        f.e_a1, f.e_hid, f.e_h = (np.where(zero, 0.0, v) for v in (e_a1, e_hid, e_h))
        f.sigma_lo, f.sigma_hi = sigma_interval(f.h[:, 0], f.e_h[:, 0])
    return f


FLT_MAX = float(np.finfo(F32).max)
FLT_MIN = 2.0 ** -126              # smallest normal fp32
EXPF_ULP = 2.0 ** -23              # libm expf: 1 ulp (module docstring)


def sigma_interval(h0, e_h0):
    """Where ``expf(h0~)`` may land for h0~ within e_h0 of h0: [exp(h0 - e)
    (1 - 2^-23), exp(h0 + e) (1 + 2^-23)] (expf: 1 ulp).  An end below 2^-126
    moves out by 2^-126 (a subnormal result may be flushed or kept: both
    pass).  ``sigma_hi`` > FLT_MAX allows +inf, ``sigma_lo`` > FLT_MAX demands
    it (``in_sigma_interval``).  An exact-zero h0 with a zero bound is
    expf(0) = 1.0 exactly.  A NaN h0 gives NaN ends."""
    h0, e = np.asarray(h0, F64), np.asarray(e_h0, F64)
    e = np.where(np.isfinite(h0), e, 0.0)          # +-inf: exp is inf / 0 whatever the bound says
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        lo = np.exp(h0 - e) * (1.0 - EXPF_ULP)
        hi = np.exp(h0 + e) * (1.0 + EXPF_ULP)
        lo = np.where(lo < FLT_MIN, np.maximum(lo - FLT_MIN, 0.0), lo)
        hi = np.where(hi < FLT_MIN, hi + FLT_MIN, hi)
    one = (h0 == 0.0) & (e == 0.0)
    return np.where(one, 1.0, lo), np.where(one, 1.0, hi)


def in_sigma_interval(got, lo, hi):
    """bool per element: ``got`` (fp32 values) allowed by the interval."""
    got = np.asarray(got, F64)
    with np.errstate(invalid="ignore"):
        finite_ok = np.isfinite(got) & (got >= lo) & (got <= hi) & ~(lo > FLT_MAX)
        inf_ok = np.isposinf(got) & (hi > FLT_MAX)
        nan_ok = np.isnan(got) & np.isnan(lo)
    return finite_ok | inf_ok | nan_ok


def sigma_backward(feat, d_h, sigma_params, mode=FP32, round_hidden=False, dt=F64,
                   mutant=()):
    """feat [M, 32] (column 2 level + c), d_h [M, 16] -> d_feat [M, 32], dW
    [3072] = [dW1 64x32 | dW2 16x64] and their bounds.  ``round_hidden`` (the
    ``_h16`` entry point): the hidden pre-activation is rounded to fp16 before
    the gate and before dW2 read it."""
    f = sigma_forward(feat, sigma_params, mode, round_hidden, dt)
    dh = np.asarray(_np(d_h, F32), dt).reshape(-1, 16)
    M = dh.shape[0]
    hid = np.maximum(f.a1, 0)
    dW2, e_dW2 = _outer(dh, np.zeros(dh.shape), hid, _relu_e(f.a1, f.e_a1), mode, dt, M)
    dhid, e = _lin(dh, np.zeros(dh.shape), f.W2.T, mode, dt)
    g = _gate(f.a1, mutant)
    dhid, e = np.where(g, dhid, 0), np.where(g, e, 0.0)
    dW1, e_dW1 = _outer(dhid, e, f.x, np.zeros(f.x.shape), mode, dt, M)
    dx, e_dx = _lin(dhid, e, f.W1.T, mode, dt)
    return NS(d_feat=dx, e_d_feat=e_dx, dW=np.concatenate([dW1.ravel(), dW2.ravel()]),
              e_dW=np.concatenate([e_dW1.ravel(), e_dW2.ravel()]), f=f)


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def worst_ratio(err, bound):
    """max err / bound with 0 / 0 = 0, x / 0 = inf and nan = inf."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


WORST = {}          # what -> worst err / bound seen (the GPU tests print it at the end)


def compare(got, ref, bound, what):
    """Every element of ``got`` within ``bound`` of ``ref``; prints the worst
    err / bound, raises above 1.  -> worst."""
    got = _np(got, F64)
    ref = np.asarray(ref, F64)
    if got.shape != ref.shape:
        raise Mismatch(f"{what}: shape {got.shape} != {ref.shape}")
    if not np.isfinite(got).all():
        raise Mismatch(f"{what}: non-finite output")
    with np.errstate(invalid="ignore"):
        worst = worst_ratio(np.abs(got - ref), bound)
    print(f"{what}: worst err/bound {worst:.3f}")
    key = what.split(" @ ")[0]
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        i = int(np.argmax(np.nan_to_num(np.abs(got - ref) / np.maximum(np.asarray(bound, F64), 1e-300), nan=np.inf, posinf=1e300)))
        raise Mismatch(f"{what}: err/bound {worst:.3g} at flat index {i}: got {got.ravel()[i]!r} "
                       f"ref {ref.ravel()[i]!r} bound {np.broadcast_to(bound, ref.shape).ravel()[i]!r}")
    return worst


def compare_exact(got, ref, what):
    got, ref = _np(got, np.int64), np.asarray(ref, np.int64)
    if got.shape != ref.shape or not np.array_equal(got, ref):
        raise Mismatch(f"{what}: differs from the reference")


def compare_forward(got, ref, what, where=""):
    """got: dict with src, weights, image, depth, semantics (any may be absent).
    ``what`` names the entry point and the case family (the key of WORST),
    ``where`` the case."""
    if "src" in got:
        compare_exact(got["src"], ref.src, f"{what} src @ {where}")
    for k in ("weights", "image", "depth", "semantics"):
        if k in got:
            compare(got[k], getattr(ref, k), getattr(ref, "e_" + k), f"{what} {k} @ {where}")


def compare_backward(got, ref, what, where=""):
    """got: dict with G, d_h_c, d_h_f, dW_color, dW_sem."""
    for k in ("G", "d_h_c", "d_h_f", "dW_color", "dW_sem"):
        if k in got and getattr(ref, k) is not None:
            compare(got[k], getattr(ref, k), getattr(ref, "e_" + k), f"{what} {k} @ {where}")


def compare_sigma(got, ref, what, where=""):
    for k in ("d_feat", "dW"):
        compare(got[k], getattr(ref, k), getattr(ref, "e_" + k), f"{what} {k} @ {where}")


# ---------------------------------------------------------------------------
# cases: synthetic stage inputs (numpy generators, fp32 arrays), the smallest
# shapes at which the kernels can still go wrong
# ---------------------------------------------------------------------------
PIN_MODES = (FP32, X2, F16M(1024.0))   # the margins a case can be pinned at
REDRAW_CAP = 0.05


class RedrawCap(AssertionError):
    pass


def _near_zero(a, e):
    """pre-activation within its bound of zero (an exact zero whose bound is
    zero -- every input zero -- is the same exact zero in the kernel)."""
    return ((np.abs(np.asarray(a, F64)) <= e) & (e > 0)).any(1)


def _gate_offenders(dirs, geo, nets_by_mode, C):
    bad = np.zeros(len(dirs), bool)
    for mode, nets in nets_by_mode:
        f = shade_forward(dirs, geo, nets, C, mode)
        for a, e in ((f.a1, f.e_a1), (f.a2, f.e_a2), (f.a1s, f.e_a1s)):
            bad |= _near_zero(a, e)
    return bad


def pin_case(c, rng, mode, sigma_draw=None):
    """Redraw the h row of every sample with a hidden pre-activation within its
    error bound of zero in ``mode`` (the float64 value; in fp16 mode the
    fp16-emulated one), then the sigma of every sample whose float64 weight is
    within its bound of 1e-4, until none is left.  -> fraction redrawn (asserted
    <= 5 %)."""
    N, T, t, C = c.N, c.T, c.t, c.C
    S = T + t
    nets = [(mode, split_nets(c.color_params, c.sem_params, C, mode))]
    c.mode = mode
    h = _rows(c.h_c, c.h_f, N, T, t).copy()                   # [N, S, 16], source order
    dirs = np.repeat(c.rays_d, S, 0)
    flat = h.reshape(N * S, 16)
    redrawn = np.zeros(N * S, bool)
    idx = np.arange(N * S)
    for _ in range(100):
        bad = _gate_offenders(dirs[idx], flat[idx, 1:], nets, C)
        idx = idx[bad]
        if idx.size == 0:
            break
        redrawn[idx] = True
        flat[idx, 1:] = rng.standard_normal((idx.size, 15)).astype(F32)
    else:
        raise AssertionError("gates not pinned after 100 rounds")
    c.h_c = np.ascontiguousarray(h[:, :T].reshape(N * T, 16))
    c.h_f = np.ascontiguousarray(h[:, T:].reshape(N * t, 16)) if t else None
    sig = c.sigma_c if t == 0 else np.concatenate([c.sigma_c, c.sigma_f], 1)
    src = merge_src(c.z_c, c.z_f)
    zs = _gather_sorted(src, T, c.z_c, c.z_f, F64)
    red_w = np.zeros((N, S), bool)
    for _ in range(100):
        sg = np.take_along_axis(sig, src.astype(np.int64), 1)
        rw = ray_weights(zs, sg, c.density_scale)
        # the kernel's threshold is the fp32 number 1e-4f, 2.6e-12 below 1e-4
        bad = np.abs(rw.w - W_MIN) <= rw.e_w + abs(W_MIN - float(F32(W_MIN)))
        if not bad.any():
            break
        red_w |= bad
        r_, s_ = np.nonzero(bad)
        new = (sigma_draw or (lambda k: np.exp(rng.standard_normal(k))))(len(r_))
        sig[r_, src[r_, s_]] = np.asarray(new, F32)
    else:
        raise AssertionError("mask not pinned after 100 rounds")
    c.sigma_c = np.ascontiguousarray(sig[:, :T])
    c.sigma_f = np.ascontiguousarray(sig[:, T:]) if t else None
    # slot 0 of an h row is the sigma net's raw output: sigma = exp(h0)
    c.h_c[:, 0] = np.log(np.maximum(c.sigma_c, F32(1e-30))).reshape(-1)
    if t:
        c.h_f[:, 0] = np.log(np.maximum(c.sigma_f, F32(1e-30))).reshape(-1)
    c.redrawn = float(np.maximum(redrawn.reshape(N, S), red_w).mean()) if N * S else 0.0
    if c.redrawn > REDRAW_CAP:
        raise RedrawCap(f"{c.name} at the {mode} margin: {c.redrawn:.1%} of the samples redrawn")
    return c.redrawn


def _inputs(name, rng, N, T, t, C, density_scale=1.0, sigma_scale=0.85):
    """Random h rows (magnitude ~1), unit directions, sorted depths in
    [0.5, 4], lognormal sigmas with an optical depth of ~3 per ray."""
    d = rng.standard_normal((N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = NS(name=name, N=N, T=T, t=t, C=C, density_scale=float(density_scale))
    c.rays_d = d.astype(F32)
    c.norms = (1.0 + 0.3 * rng.random(N)).astype(F32)
    c.z_c = np.sort(0.5 + 3.5 * rng.random((N, T)), 1).astype(F32)
    c.z_f = np.sort(0.5 + 3.5 * rng.random((N, t)), 1).astype(F32) if t else None
    c.sigma_c = (sigma_scale / density_scale * np.exp(0.7 * rng.standard_normal((N, T)))).astype(F32)
    c.sigma_f = (sigma_scale / density_scale * np.exp(0.7 * rng.standard_normal((N, t)))).astype(F32) if t else None
    c.h_c = rng.standard_normal((N * T, 16)).astype(F32)
    c.h_f = rng.standard_normal((N * t, 16)).astype(F32) if t else None
    c.d_image = rng.standard_normal((N, 3)).astype(F32)
    c.d_depth = rng.standard_normal(N).astype(F32)
    c.d_sem = rng.standard_normal((N, C)).astype(F32)
    return c


def _set_sorted_sigma(c, sg_sorted):
    """write sigmas given in depth order back to their [coarse | fine] slots"""
    src = merge_src(c.z_c, c.z_f).astype(np.int64)
    sig = np.zeros((c.N, c.T + c.t), F32)
    np.put_along_axis(sig, src, np.asarray(sg_sorted, F32), 1)
    c.sigma_c = np.ascontiguousarray(sig[:, :c.T])
    c.sigma_f = np.ascontiguousarray(sig[:, c.T:]) if c.t else None


def _sigma_for_alpha(c, alpha_sorted):
    src = merge_src(c.z_c, c.z_f)
    zs = _gather_sorted(src, c.T, c.z_c, c.z_f, F64)
    delta = np.concatenate([np.diff(zs, axis=1), np.full((c.N, 1), 1e10)], 1)
    delta = np.maximum(delta, 1e-6)
    return -np.log1p(-np.asarray(alpha_sorted, F64)) / (delta * c.density_scale)


BLOCK_COUNTS = (15, 1, 15, 17, 31, 33, 0, 64, 1, 0, 16, 16, 32, 15, 17, 31, 33, 0,
                0, 0, 64, 64, 15)
LONG_SHAPES = ((64, 0), (33, 32), (96, 34), (256, 256))
CLASS_COUNTS = (1, 15, 16, 17, 40, 61)
TAIL_N = (1, 2, 3, 17, 131)
SIGMA_M = (1, 15, 16, 17, 63, 64, 65, 255, 257, 2049)


def case_tails(color_params, sem_params, mode, N, C=40, seed=0):
    rng = np.random.default_rng(1000 + N + seed)
    c = _inputs(f"tails[{N}]", rng, N, 16, 16, C)
    c.color_params, c.sem_params = color_params, sem_params
    pin_case(c, rng, mode, lambda k: 0.85 * np.exp(0.7 * rng.standard_normal(k)))
    return c


def case_blocks(color_params, sem_params, mode, C=40, seed=0):
    """One ray per survivor count, S = 70.  A wave shades two consecutive rays
    through one pending list: (15, 1) and (15, 17) complete a 16-block with the
    next ray's first survivor, (31, 33), (17, 31), (32, 15) straddle likewise,
    (0, 64) fills the list from empty, some rays and one whole wave are empty."""
    rng = np.random.default_rng(2000 + seed)
    N = len(BLOCK_COUNTS)
    c = _inputs("blocks", rng, N, 35, 35, C)
    c.color_params, c.sem_params = color_params, sem_params
    S = 70
    alpha = np.zeros((N, S))
    for r, k in enumerate(BLOCK_COUNTS):
        pos = np.sort(rng.choice(S - 1, k, replace=False))     # never the 1e10-wide last one
        alpha[r, pos] = 0.02 + 0.03 * rng.random(k)
    _set_sorted_sigma(c, _sigma_for_alpha(c, alpha))
    pin_case(c, rng, mode)
    got = composite_forward(*forward_args(c)).mask.sum(1)
    assert tuple(got) == BLOCK_COUNTS, got
    return c


def case_long(color_params, sem_params, mode, T, t, C=40, seed=0):
    """S = 64, 65, 130, 512: the scan carries; rays 0..4 keep EVERY sample
    (alpha ~ 2 / S each: all 64 of a pass join a pending list that may already
    hold 15), the others are random."""
    rng = np.random.default_rng(3000 + T + t + seed)
    N = 9
    c = _inputs(f"long[{T},{t}]", rng, N, T, t, C, sigma_scale=0.85)
    c.color_params, c.sem_params = color_params, sem_params
    S = T + t
    src = merge_src(c.z_c, c.z_f).astype(np.int64)
    sg = np.take_along_axis(np.concatenate([c.sigma_c] + ([c.sigma_f] if t else []), 1), src, 1)
    dense = _sigma_for_alpha(c, (1.5 + rng.random((N, S))) / S)
    dense[:, -1] = sg[:, -1]
    sg[:5] = dense[:5]
    _set_sorted_sigma(c, sg)
    pin_case(c, rng, mode)
    return c


def case_weights(color_params, sem_params, mode, C=40, seed=0):
    """N = 8, T = 24, t = 40, density_scale = 0.25.  Ray 0, 1: an opaque sample
    in mid-ray (sigma delta scale > 1000: expf underflows to exactly 0, fac is
    the bare 1e-15).  Ray 2: sigmas below e^-15; ray 3: above e^15 on a thin
    interval and moderate elsewhere.  Ray 4, 5: a fine depth bit-equal to a
    coarse one (a zero delta).  Ray 6: two equal coarse depths.  Ray 7: plain."""
    rng = np.random.default_rng(4000 + seed)
    N, T, t = 8, 24, 40
    c = _inputs("weights", rng, N, T, t, C, density_scale=0.25)
    c.color_params, c.sem_params = color_params, sem_params
    c.z_f[4, 7], c.z_f[5, 20] = c.z_c[4, 5], c.z_c[5, 11]
    c.z_f[4].sort()
    c.z_f[5].sort()
    c.z_c[6, 9] = c.z_c[6, 8]
    src = merge_src(c.z_c, c.z_f).astype(np.int64)
    zs = _gather_sorted(src, T, c.z_c, c.z_f, F64)
    delta = np.maximum(np.diff(zs, axis=1), 1e-6)
    sg = np.take_along_axis(np.concatenate([c.sigma_c, c.sigma_f], 1), src, 1).astype(F64)
    for r, s in ((0, 30), (1, 12)):
        sg[r, s] = 4000.0 / (delta[r, s] * 0.25)
    sg[2, ::3] = math.exp(-16.0) * (0.5 + rng.random(len(sg[2, ::3])))
    # sigma = e^15.5 on an interval an ulp or two wide, so that it is not opaque
    s = 20
    e = src[3, s + 1]
    (c.z_c if e < T else c.z_f)[3, e if e < T else e - T] = F32(zs[3, s] + 0.5 / (0.25 * math.exp(15.5)))
    sg[3, s] = math.exp(15.5)
    c.special = dict(opaque=((0, 30), (1, 12)), tiny_row=2, huge=(3, s))
    _set_sorted_sigma(c, sg)
    pin_case(c, rng, mode)
    return c


def case_classes(color_params, sem_params, mode, C, seed=0):
    rng = np.random.default_rng(5000 + C + seed)
    c = _inputs(f"classes[{C}]", rng, 17, 16, 16, C)
    c.color_params, c.sem_params = color_params, sem_params
    pin_case(c, rng, mode)
    return c


def case_t0(color_params, sem_params, mode, C=40, seed=0):
    rng = np.random.default_rng(6000 + seed)
    c = _inputs("t0", rng, 17, 24, 0, C)
    c.color_params, c.sem_params = color_params, sem_params
    pin_case(c, rng, mode)
    return c


def case_sigma(sigma_params, M, seed=0):
    """feat [M, 32] ~ N(0, 1), d_h [M, 16] ~ N(0, 1) with a tenth of the rows
    zero; from M = 15 on one feat row is all zero (every pre-activation exactly
    0: the gate must be closed).  Rows with a hidden pre-activation within its
    bound of zero (fp32, bf16x2, and the fp16-rounded hidden layer) are
    redrawn, at most 5 %."""
    rng = np.random.default_rng(7000 + M + seed)
    c = NS(name=f"sigma[{M}]", M=M, sigma_params=sigma_params)
    feat = rng.standard_normal((M, 32)).astype(F32)
    d_h = rng.standard_normal((M, 16)).astype(F32)
    d_h[rng.random(M) < 0.1] = 0
    if M >= 15:
        feat[M // 2] = 0
        d_h[M // 2] = rng.standard_normal(16).astype(F32)
    idx = np.arange(M)
    red = np.zeros(M, bool)
    for _ in range(100):
        bad = np.zeros(idx.size, bool)
        for mode, rh in ((FP32, False), (X2, False), (FP32, True)):
            f = sigma_forward(feat[idx], sigma_params, mode, rh)
            bad |= _near_zero(f.a1, f.e_a1)
        idx = idx[bad]
        if idx.size == 0:
            break
        red[idx] = True
        feat[idx] = rng.standard_normal((idx.size, 32)).astype(F32)
    else:
        raise AssertionError("sigma gates not pinned")
    c.feat, c.d_h = feat, d_h
    c.redrawn = float(red.mean())
    if c.redrawn > REDRAW_CAP:
        raise RedrawCap(f"{c.name}: {c.redrawn:.1%} of the rows redrawn")
    return c


def all_case_specs():
    """(family, key, builder arguments) of every composite case the GPU tests run."""
    specs = [("tails", N, dict(N=N)) for N in TAIL_N]
    specs.append(("blocks", None, {}))
    specs += [("long", (T, t), dict(T=T, t=t)) for T, t in LONG_SHAPES]
    specs.append(("weights", None, {}))
    specs += [("classes", C, dict(C=C)) for C in CLASS_COUNTS]
    specs.append(("t0", None, {}))
    return specs


def build_sigma_case(sigma_params, M):
    """as ``build_case``: the first seed whose redraws stay under the cap"""
    for k in range(8):
        try:
            return case_sigma(sigma_params, M, seed=10000 * k)
        except RedrawCap:
            continue
    raise RedrawCap(f"sigma[{M}]: no seed of 8 met the redraw cap")


BUILDERS = dict(tails=case_tails, blocks=case_blocks, long=case_long,
                weights=case_weights, classes=case_classes, t0=case_t0)


def build_case(family, color_params, sem_params, mode, **kw):
    """The family's case pinned at ``mode``'s margin.  The bf16x2 margin (2^-16
    per product through two layers, worst case) catches ~4 % of random rows, so
    a small case can exceed the 5 % cap by chance: the builder's generator is
    then re-seeded (seed = 10000, 20000, ...) and the case is the FIRST one the
    reference alone accepts; the cap itself is asserted on what is returned."""
    for k in range(8):
        try:
            c = BUILDERS[family](color_params, sem_params, mode, seed=10000 * k, **kw)
        except RedrawCap:
            continue
        assert c.redrawn <= REDRAW_CAP
        c.reseeded = k
        return c
    raise RedrawCap(f"{family} {kw}: no seed of 8 met the {REDRAW_CAP:.0%} redraw cap at the {mode} margin")


def forward_args(c):
    return (c.rays_d, c.norms, c.z_c, c.sigma_c, c.h_c, c.z_f, c.sigma_f, c.h_f,
            c.color_params, c.sem_params, c.C, c.density_scale)
