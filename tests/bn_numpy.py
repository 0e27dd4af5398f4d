"""numpy restatement of the fused BatchNorm2d (+ residual) (+ ReLU) contract of
include/ucsa_hip.h (``ucsa_bn_act_fwd`` / ``ucsa_bn_act_bwd``, csrc/batchnorm.hip)
in float64, with a derived bound on |kernel - reference| for every output: the
yardstick of tests/test_bn_reference_cpu.py and tests/test_gpu_bn_reference.py
(test infrastructure: plain numpy, no torch, no GPU, no HIP library).

Everything works on ``[M, C]`` arrays (an NHWC activation is that matrix), whose
values are the exact fp32 or bf16 inputs widened to float64.  ``eps`` and
``momentum`` are the fp32 numbers the entry point receives (rounded here).

Bounds, u = 2^-24 (fp32 round to nearest), gamma_n = n u / (1 - n u):

* Sums.  ``bn_geom`` is restated in ``geom``: a thread adds
  ``n_chain = rows_per_wg / rows_per_it`` terms one after the other (the 4-way and
  2-way unrolling keeps that order), an LDS tree of ``log2(rows_per_it)`` levels
  follows: a term passes through at most ``depth = n_chain + levels`` fp32
  additions, whatever the order, so |sum^ - sum| <= gamma_(depth + k) sum|term|
  with k the roundings inside a term (x - shift: 1; its square: 3; g xhat: 3).
  The per-workgroup partials are combined in double (<= 128 + 8 additions of
  2^-53 each): negligible, covered by the factor ``SECOND`` below.
* Variance and invstd.  var = SS / M - m1^2 with m1 = S1 / M the mean of
  x - shift: e_var = e_SS / M + 2 |m1| e_m1 + e_m1^2, which grows with
  ((mean - shift) / std)^2 on its own.  invstd = (var + eps)^-1/2 is monotone:
  e_invstd is the larger of its changes at max(var - e_var, 0) (the kernel
  clamps at 0 too) and at var + e_var, plus the rounding to fp32.  running_var
  takes the unbiased variance var M / (M - 1), or var itself when M = 1 (the
  kernel's rule).
* y.  The kernel evaluates a^ x + b^ with a^ = fl(gamma invstd^),
  b^ = fl(beta - fl(mean^ a^)), i.e. a^ (x - mean^) + beta up to roundings:
  e_pre = e_a |x - mean| + (|a| + e_a) e_mean
          + u (|mean a| + |b| + |a x| + |a x + b| + |pre|),
  one u per rounded operation whether or not the compiler contracts a
  multiply-add (a contraction removes a rounding).  A channel whose invstd is
  poorly determined (nearly constant: |x - mean| tiny) still gets a tight bound.
  ReLU is 1-Lipschitz, and an element whose pre-activation is more than its
  bound below 0 is exactly 0 on both sides (bound 0); the builders pin every
  pre-activation at least 4 bounds away from 0, so that is every element that
  is off.
* Eval mode.  invstd = 1 / sqrtf(running_var + eps) in fp32: the addition (u,
  halved by the root), the root and the division (<= 1 ulp = 2 u each): 5 u.
* dx.  The kernel evaluates kg g + kx x + k0 with three coefficients rounded to
  fp32 from double: the error of the two sums enters as
  |c1 invstd| e_sgx / M |x - mean| + |c1| e_sg / M (kx and k0 share the same
  double), the roundings as u (2 |c1 g| + 2 |kx x| + |k0| + |c1 g - kx x| + |dx|):
  u (|kx x| + |k0|) is what a large mean / std costs.
* dresidual = g is a copy: bound 0 in both types.
* bf16.  y and dx are stored round-to-nearest-even: + half a bf16 ulp of the
  value, 2^(floor(log2 |v|) - 8) with |v| taken as |value| + e.  (bf16 keeps 8
  significant bits, so half an ulp is 2^-9 of the power of two ABOVE |v| and
  at most 2^-8 |v|; "2^-9 |v|" is not attainable by rounding to nearest.  A
  truncating store errs by up to a whole ulp and is rejected.)

No safety factor is applied: the only slack is ``SECOND`` = 1 + 2^-20 for the
second-order terms (products of two roundings, the double arithmetic).

``emulate_forward`` / ``emulate_backward`` evaluate the same contract in fp32 in
the kernels' own summation order (per-thread strided chains, LDS tree, double
combine) and coefficient arithmetic; ``mutant`` names one deliberate mistake.
"""
import math
from types import SimpleNamespace as NS

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -149
SECOND = 1.0 + 2.0 ** -20
BN_THREADS = 256
APPLY_QUADS = 8192 * 256            # quads of one grid-stride pass of the apply kernels
SUB = {"f32": 2.0 ** -149, "bf16": 2.0 ** -133}   # smallest positive subnormal

MUTANTS = ("biased_running_var", "unbiased_normalises", "momentum_swapped", "eps_outside_sqrt",
           "shift_not_added", "running_mean_shifted", "res_after_relu", "mask_from_x", "mask_ge",
           "dres_unmasked", "dgamma_from_x", "dx_no_mean_g", "dx_no_xhat", "dx_m_minus_1",
           "tail_rows_dropped", "last_wg_dropped", "quads_swapped", "second_pass_skipped",
           "bf16_truncated", "nan_zeroed")


def gamma_n(n):
    return n * U / (1.0 - n * U)


def geom(M, C):
    """``bn_geom`` of csrc/batchnorm.hip."""
    cq = C // 4
    tq = 1
    while tq < 16 and tq * 2 <= cq and cq % (tq * 2) == 0:
        tq *= 2
    rpi = BN_THREADS // tq
    n_col_wg = cq // tq
    want = min(max(2048 // n_col_wg, 1), 128)
    rows = max((M + want - 1) // want, 4 * rpi)
    rows = (rows + rpi - 1) // rpi * rpi
    n_chain, levels = rows // rpi, int(math.log2(rpi))
    return NS(M=M, C=C, tq=tq, rows_per_it=rpi, rows_per_wg=rows, n_row_wg=(M + rows - 1) // rows,
              n_col_wg=n_col_wg, n_chain=n_chain, levels=levels, depth=n_chain + levels)


def bf16_round(a, truncate=False):
    """fp32 array -> the nearest-even (or truncated) bf16 value, as fp32."""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    if not truncate:
        b = b + (np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1)))
    out = (b & np.uint32(0xFFFF0000)).view(F32)
    return np.where(np.isnan(a), F32(np.nan), out).astype(F32)


def to_dtype(a, dtype):
    a = np.asarray(a, F64).astype(F32)
    return bf16_round(a) if dtype == "bf16" else a


def _d(a):
    return None if a is None else np.asarray(a, F64)


def _rnd(v, e):
    """bound after rounding to fp32 a value within e of v"""
    return e + U * (np.abs(v) + e)


def half_ulp_bf16(m):
    """half an ulp of bf16 at magnitude m >= 0 (0 at 0; 2^-134 among the subnormals)"""
    m = np.asarray(m, F64)
    with np.errstate(invalid="ignore"):
        _, ex = np.frexp(np.where(np.isfinite(m), m, 1.0))
    h = np.maximum(np.ldexp(1.0, ex - 9), 2.0 ** -134)
    return np.where(m == 0, 0.0, np.where(np.isfinite(m), h, np.inf))


def _store(v, e, dtype):
    return e + half_ulp_bf16(np.abs(v) + e) if dtype == "bf16" else e


# ---------------------------------------------------------------------------
# the float64 restatement
# ---------------------------------------------------------------------------
def forward(x, res, gamma, beta, running_mean, running_var, momentum, eps, relu, training,
            dtype="f32", round_args=True, model="kernel"):
    """-> y, save_mean, save_invstd, new_running_mean, new_running_var (None where
    the entry point writes none), ``pre`` (before the ReLU) and ``e_*`` bounds.
    ``round_args=False`` keeps eps and momentum as doubles (to compare with torch
    in double, which does).  ``model="generic"`` gives the bounds of the same
    formulas for an fp32 implementation that does NOT share the kernels'
    geometry: no shift, sums of any order (depth M), and the running-statistics
    update evaluated in fp32 (two products and a sum) instead of in double."""
    x, res = _d(x), _d(res)
    M, C = x.shape
    g = geom(M, C)
    gam = np.ones(C) if gamma is None else _d(gamma)
    bet = np.zeros(C) if beta is None else _d(beta)
    eps, mom = (float(F32(eps)), float(F32(momentum))) if round_args else (float(eps), float(momentum))
    r = NS(geom=g, save_mean=None, save_invstd=None, new_running_mean=None, new_running_var=None)
    with np.errstate(invalid="ignore", over="ignore"):
        if training:
            depth = g.depth if model == "kernel" else M
            old = np.zeros(C) if running_mean is None else _d(running_mean)
            s = old if model == "kernel" else np.zeros(C)
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
            d = x - s
            m1 = mean - s
            e_m1 = gamma_n(depth + 1) * np.abs(d).sum(0) / M
            e_ss = gamma_n(depth + 3) * (d * d).sum(0) / M + TINY
            e_var = e_ss + 2.0 * np.abs(m1) * e_m1 + e_m1 ** 2
            invstd = 1.0 / np.sqrt(var + eps)
            e_invstd = _rnd(invstd, np.maximum(1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps) - invstd,
                                               invstd - 1.0 / np.sqrt(var + e_var + eps)))
            e_mean = _rnd(mean, e_m1)
            r.save_mean, r.e_save_mean, r.save_invstd, r.e_save_invstd = mean, e_mean, invstd, e_invstd
            r.e_var = e_var
            if running_mean is not None:
                fac = M / (M - 1.0) if M > 1 else 1.0
                upd = 0.0 if model == "kernel" else 3.0 * U
                r.new_running_mean = (1.0 - mom) * old + mom * mean
                r.e_new_running_mean = _rnd(r.new_running_mean, mom * e_m1 + upd * (
                    np.abs((1.0 - mom) * old) + np.abs(mom * mean)))
                r.new_running_var = (1.0 - mom) * _d(running_var) + mom * var * fac
                r.e_new_running_var = _rnd(r.new_running_var, mom * fac * e_var + upd * r.new_running_var)
        else:
            mean, e_mean = _d(running_mean), np.zeros(C)
            invstd = 1.0 / np.sqrt(_d(running_var) + eps)
            e_invstd = 5.0 * U * invstd
        a = gam * invstd
        e_a = np.abs(gam) * e_invstd + U * np.abs(a)
        p = mean * a
        b = bet - p
        pre0 = a * (x - mean) + bet
        pre = pre0 if res is None else pre0 + res
        mags = np.abs(p) + np.abs(b) + np.abs(a * x) + np.abs(pre0)
        if res is not None:
            mags = mags + np.abs(pre)
        e_pre = (e_a * np.abs(x - mean) + (np.abs(a) + e_a) * e_mean + U * mags) * SECOND
        r.pre, r.e_pre = pre, e_pre
        if relu:
            r.y = np.maximum(pre, 0.0)                       # propagates NaN
            r.e_y = np.where(pre < -e_pre, 0.0, _store(r.y, e_pre, dtype))
        else:
            r.y, r.e_y = pre, _store(pre, e_pre, dtype)
    r.mean, r.invstd = mean, invstd
    return r


def backward(dy, x, y, gamma, mean, invstd, relu, dtype="f32", model="kernel"):
    """-> dx, dres (= g), dgamma, dbeta and their bounds.  ``mean`` / ``invstd``
    are the fp32 vectors the entry point receives, whatever they are."""
    dy, x, mean, invstd = _d(dy), _d(x), _d(mean), _d(invstd)
    M, C = x.shape
    g = geom(M, C)
    gam = np.ones(C) if gamma is None else _d(gamma)
    gv = np.where(_d(y) > 0, dy, 0.0) if relu else dy
    xh = (x - mean) * invstd
    sg, sgx = gv.sum(0), (gv * xh).sum(0)
    depth = g.depth if model == "kernel" else M
    e_sg = gamma_n(depth) * np.abs(gv).sum(0)
    e_sgx = gamma_n(depth + 3) * np.abs(gv * xh).sum(0) + M * TINY
    c1 = gam * invstd
    kx = c1 * (sgx / M) * invstd
    k0 = kx * mean - c1 * (sg / M)
    t1, t2 = c1 * gv, kx * x
    dx = c1 * (gv - sg / M - xh * (sgx / M))
    e = (np.abs(c1 * invstd) * (e_sgx / M) * np.abs(x - mean) + np.abs(c1) * (e_sg / M)
         + U * (2.0 * np.abs(t1) + 2.0 * np.abs(t2) + np.abs(k0) + np.abs(t1 - t2) + np.abs(dx))) * SECOND + TINY
    return NS(geom=g, dx=dx, e_dx=_store(dx, e, dtype), dres=gv, e_dres=np.zeros_like(gv),
              dgamma=sgx, e_dgamma=_rnd(sgx, e_sgx) * SECOND, dbeta=sg, e_dbeta=_rnd(sg, e_sg) * SECOND)


def eval_backward(dy, x, y, gamma, running_mean, running_var, eps, relu, dtype="f32"):
    """The eval-mode backward of ``_BnActFn`` (plain torch, fp32 statistics):
    dx = g * k with k = gamma * rsqrt(running_var + eps) ROUNDED TO THE
    ACTIVATION'S TYPE before the product (bf16: half an ulp of k, then half an
    ulp of the product), rsqrt of an fp32 sum: 4 u; dgamma = sum g xhat and dbeta = sum g in
    fp32 by torch's reduction (any order: M u of the absolute sum)."""
    dy, x = _d(dy), _d(x)
    M, C = x.shape
    eps = float(F32(eps))
    gam = np.ones(C) if gamma is None else _d(gamma)
    gv = np.where(_d(y) > 0, dy, 0.0) if relu else dy
    invstd = 1.0 / np.sqrt(_d(running_var) + eps)
    k = gam * invstd
    e_k = 5.0 * U * np.abs(k)
    if dtype == "bf16":
        e_k = e_k + half_ulp_bf16(np.abs(k) + e_k)
    dx = gv * k
    e_dx = _store(dx, np.abs(gv) * e_k + U * np.abs(dx), dtype)
    xh = (x - _d(running_mean)) * invstd
    return NS(dx=dx, e_dx=e_dx, dres=gv, e_dres=np.zeros_like(gv),
              dgamma=(gv * xh).sum(0), e_dgamma=gamma_n(M + 8) * np.abs(gv * xh).sum(0) + M * TINY,
              dbeta=gv.sum(0), e_dbeta=gamma_n(M + 1) * np.abs(gv).sum(0))


# ---------------------------------------------------------------------------
# fp32 emulation of the kernels (and its mutants)
# ---------------------------------------------------------------------------
def _kernel_sums(terms, g, mutant, unroll):
    """Column sums of fp32 [M, C] arrays in the order of k_bn_stats /
    k_bn_bwd_stats + bn_group_reduce: thread rr of workgroup w adds rows
    w rows_per_wg + rr + k rows_per_it in sequence, the LDS tree halves over rr,
    the per-workgroup fp32 partials are added in double."""
    M, C, W, R, n_it = g.M, g.C, g.n_row_wg, g.rows_per_it, g.n_chain
    row = np.arange(W * n_it * R).reshape(W, n_it, R)
    valid = row < M
    if "tail_rows_dropped" in mutant:
        cnt = valid.sum(1)                                    # rows of each thread
        valid &= np.arange(n_it)[None, :, None] < (cnt // unroll * unroll)[:, None, :]
    out = []
    for t in terms:
        pad = np.zeros((W * n_it * R, C), F32)
        pad[:M] = t
        pad = pad.reshape(W, n_it, R, C)
        acc = np.zeros((W, R, C), F32)
        with np.errstate(invalid="ignore", over="ignore"):
            for it in range(n_it):
                acc = acc + np.where(valid[:, it, :, None], pad[:, it], F32(0))
            n = R
            while n > 1:
                h = n // 2
                acc[:, :h] = acc[:, :h] + acc[:, h:n]
                n = h
        part = acc[:, 0].astype(F64)
        if "last_wg_dropped" in mutant:
            part = part[:-1]
        out.append(part.sum(0))
    return out


def _emu_store(v, dtype, mutant, swap=True):
    """what the apply kernels leave in memory: v [M, C] fp32 (quads beyond one
    grid-stride pass unwritten = 0 under ``second_pass_skipped``)"""
    v = np.array(v, F32)
    if "quads_swapped" in mutant and v.shape[1] >= 8 and swap:
        v[:, :8] = np.concatenate([v[:, 4:8], v[:, :4]], 1)
    if "second_pass_skipped" in mutant:
        v.reshape(-1)[APPLY_QUADS * 4:] = 0
    if dtype == "bf16":
        v = bf16_round(v, truncate="bf16_truncated" in mutant)
    return v.astype(F64)


def emulate_forward(x, res, gamma, beta, running_mean, running_var, momentum, eps, relu, training,
                    dtype="f32", mutant=(), nan_keeps=True):
    x32 = np.asarray(x, F32)
    M, C = x32.shape
    g = geom(M, C)
    gam = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    bet = np.zeros(C, F32) if beta is None else np.asarray(beta, F32)
    eps, mom = float(F32(eps)), float(F32(momentum))
    r = NS(save_mean=None, save_invstd=None, new_running_mean=None, new_running_var=None)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if training:
            sh32 = np.zeros(C, F32) if running_mean is None else np.asarray(running_mean, F32)
            d = x32 - sh32
            s1, ss = _kernel_sums([d, d * d], g, mutant, 4)
            shf = sh32.astype(F64)
            m1 = s1 / M
            var = np.maximum(ss / M - m1 * m1, 0.0)
            var = np.where(np.isnan(ss / M - m1 * m1), np.nan, var)
            mean = m1 + shf
            unb = var * (M / (M - 1.0)) if M > 1 and "biased_running_var" not in mutant else var
            nv = unb if "unbiased_normalises" in mutant else var
            inv = 1.0 / (np.sqrt(nv) + eps) if "eps_outside_sqrt" in mutant else 1.0 / np.sqrt(nv + eps)
            invstd, mf = inv.astype(F32), mean.astype(F32)
            r.save_mean = (m1 if "shift_not_added" in mutant else mean).astype(F32).astype(F64)
            r.save_invstd = invstd.astype(F64)
            if running_mean is not None:
                w_old, w_new = (mom, 1.0 - mom) if "momentum_swapped" in mutant else (1.0 - mom, mom)
                m_new = m1 if "running_mean_shifted" in mutant else mean
                r.new_running_mean = (w_old * shf + w_new * m_new).astype(F32).astype(F64)
                r.new_running_var = (w_old * np.asarray(running_var, F64) + w_new * unb).astype(F32).astype(F64)
        else:
            mf = np.asarray(running_mean, F32)
            invstd = F32(1.0) / np.sqrt(np.asarray(running_var, F32) + F32(eps))
        a = gam * invstd
        b = bet - mf * a
        v = x32 * a + b
        relu_f = (lambda t: np.where(t > 0, t, F32(0))) if "nan_zeroed" in mutant else \
            (lambda t: np.where(t < 0, F32(0), t))
        if res is not None and "res_after_relu" not in mutant:
            v = v + np.asarray(res, F32)
        if relu:
            v = relu_f(v)
        if res is not None and "res_after_relu" in mutant:
            v = v + np.asarray(res, F32)
    r.y = _emu_store(v, dtype, mutant)
    return r


def emulate_backward(dy, x, y, gamma, mean, invstd, relu, dtype="f32", mutant=()):
    dy32, x32 = np.asarray(dy, F32), np.asarray(x, F32)
    M, C = x32.shape
    g = geom(M, C)
    gam = np.ones(C, F32) if gamma is None else np.asarray(gamma, F32)
    mu, isd = np.asarray(mean, F32), np.asarray(invstd, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        gv = dy32
        if relu:
            src = x32 if "mask_from_x" in mutant else np.asarray(y, F32)
            gv = np.where(src >= 0 if "mask_ge" in mutant else src > 0, dy32, F32(0))
        xh = x32 if "dgamma_from_x" in mutant else (x32 - mu) * isd
        sg, sgx = _kernel_sums([gv, gv * xh], g, mutant, 2)
        Md = float(M - 1 if "dx_m_minus_1" in mutant else M)
        c1 = gam.astype(F64) * isd.astype(F64)
        kx = c1 * (sgx / Md) * isd.astype(F64)
        if "dx_no_xhat" in mutant:
            kx = kx * 0.0
        k0 = kx * mu.astype(F64) - (0.0 if "dx_no_mean_g" in mutant else c1 * (sg / Md))
        kg32, kx32, k032 = c1.astype(F32), (-kx).astype(F32), k0.astype(F32)
        dx = kg32 * gv + kx32 * x32 + k032
    dres = dy32 if "dres_unmasked" in mutant else gv
    return NS(dx=_emu_store(dx, dtype, mutant), dres=_emu_store(dres, dtype, mutant, swap=False),
              dgamma=sgx.astype(F32).astype(F64), dbeta=sg.astype(F32).astype(F64))


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


WORST = {}          # "entry dtype family output" -> worst err / bound seen


def worst_ratio(err, bound):
    """max err / bound with 0 / 0 = 0, x / 0 = inf and nan = inf."""
    err, bound = np.asarray(err, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.where(np.isnan(r), np.inf, r).max())


def compare(got, ref, bound, what, record=True):
    """Every element of ``got`` within ``bound`` of ``ref`` (all finite); raises
    above 1.  ``what`` = "key @ case": the key indexes WORST."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if got.shape != ref.shape:
        raise Mismatch(f"{what}: shape {got.shape} != {ref.shape}")
    if not np.isfinite(got).all():
        raise Mismatch(f"{what}: non-finite output")
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    worst = worst_ratio(err, bound)
    if record:
        key = what.split(" @ ")[0]
        WORST[key] = max(WORST.get(key, 0.0), worst)
        print(f"{what}: worst err/bound {worst:.3f}")
    if not worst <= 1.0:
        bb = np.broadcast_to(np.asarray(bound, F64), ref.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            i = int(np.argmax(np.nan_to_num(np.where(err == 0, 0.0, err / bb), nan=np.inf, posinf=1e300)))
        raise Mismatch(f"{what}: err/bound {worst:.3g} at flat index {i}: got {got.ravel()[i]!r} "
                       f"ref {ref.ravel()[i]!r} bound {bb.ravel()[i]!r}")
    return worst


FWD_OUT = ("y", "save_mean", "save_invstd", "new_running_mean", "new_running_var")
BWD_OUT = ("dx", "dres", "dgamma", "dbeta")


def compare_outputs(names, got, ref, what, where, record):
    get = (lambda k: got.get(k)) if isinstance(got, dict) else (lambda k: getattr(got, k, None))
    for k in names:
        want = getattr(ref, k)
        if (get(k) is None) != (want is None):
            raise Mismatch(f"{what} {k} @ {where}: present on one side only")
        if want is not None:
            compare(get(k), want, getattr(ref, "e_" + k), f"{what} {k} @ {where}", record)


def compare_forward(got, ref, what, where="", record=True):
    """got: dict or namespace with the five forward outputs, [M, C] / [C] (None
    where the reference has None: eval mode, no running statistics)."""
    compare_outputs(FWD_OUT, got, ref, what, where, record)


def compare_backward(got, ref, what, where="", record=True, names=BWD_OUT):
    compare_outputs(names, got, ref, what, where, record)


def compare_nan_forward(got_y, got_mean, case, ref):
    """training mode, one NaN in x[row, ch]: every y of that channel is NaN and
    so is save_mean; the other channels are inside their bounds."""
    row, ch = case.nan_at
    y = np.asarray(got_y, F64)
    if not np.isnan(y[:, ch]).all():
        raise Mismatch(f"{case.name}: {int((~np.isnan(y[:, ch])).sum())} of {y.shape[0]} outputs of the "
                       "NaN channel are not NaN")
    if not np.isnan(np.asarray(got_mean, F64)[ch]):
        raise Mismatch(f"{case.name}: save_mean of the NaN channel is not NaN")
    keep = np.arange(y.shape[1]) != ch
    compare(y[:, keep], ref.y[:, keep], ref.e_y[:, keep], f"nan y @ {case.name}", record=False)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
COLUMN_C = (4, 8, 12, 16, 24, 32, 64, 72, 136, 4096)
ROW_M64 = (1, 2, 15, 16, 17, 63, 64, 65, 129)
ROW_M4 = (255, 257, 1023, 1025)
CAP_M = (8191, 8192, 8193)
STRIDE_SHAPE = (2, 64, 257, 256)
# (residual, relu, affine, running statistics, momentum): spread over the cases
FWD_FLAGS = ((True, True, True, True, 0.1), (False, True, True, True, 0.0),
             (True, False, False, True, 1.0), (False, False, True, False, 0.1),
             (True, True, True, False, 0.1), (False, True, False, True, 1.0 / 3.0))
# (dresidual wanted, dgamma / dbeta wanted)
BWD_FLAGS = ((True, True), (False, True), (True, False), (False, False))


def _shape_specs():
    specs = [("column", f"C{C}", (1, C, 1, 70)) for C in COLUMN_C]
    specs += [("row", f"C64-M{M}", (1, 64, 1, M)) for M in ROW_M64]
    specs += [("row", f"C4-M{M}", (1, 4, 1, M)) for M in ROW_M4]
    specs += [("cap", f"M{M}", (1, 64, 1, M)) for M in CAP_M]
    specs.append(("stride", "2x64x257x256", STRIDE_SHAPE))
    return specs


SHAPE_SPECS = _shape_specs()
SHAPE_NAMES = [f"{f}-{k}" for f, k, _ in SHAPE_SPECS]
EVAL_NAMES = ("eval-C72-M70", "eval-C64-M129", "eval-C8-M257")
OFFSET_RATIOS = (0.0, 10.0, 100.0, 1000.0)
OFFSET_NAMES = ("offset-rm0", "offset-null", "offset-settled")
SYNTH_NAMES = ("synth-mean1000", "synth-corr", "synth-orth")


def _draw_forward(c, rng, mean=0.3, std=1.7):
    M, C = c.M, c.C
    res, relu, affine, stats, mom = c.flags
    c.x = to_dtype(rng.standard_normal((M, C)) * std + mean, c.dtype)
    c.res = to_dtype(rng.standard_normal((M, C)), c.dtype) if res else None
    c.gamma = (0.5 + rng.random(C)).astype(F32) * np.where(rng.random(C) < 0.25, -1, 1).astype(F32) if affine else None
    c.beta = (rng.random(C) - 0.5).astype(F32) if affine else None
    c.running_mean = (mean + 0.4 * (rng.random(C) - 0.5)).astype(F32) if stats else None
    c.running_var = (0.5 + rng.random(C)).astype(F32) if stats else None
    c.momentum, c.eps, c.relu, c.training = mom, 1e-5, relu, True


def forward_args(c):
    return (c.x, c.res, c.gamma, c.beta, c.running_mean, c.running_var, c.momentum, c.eps,
            c.relu, c.training)


def ref_forward(c, model="kernel"):
    return forward(*forward_args(c), dtype=c.dtype, model=model)


def pin_relu(c):
    """Move every pre-activation of a ReLU case at least 4 bounds away from 0
    (the residual is nudged where there is one, else x, and the statistics are
    recomputed): no exempt elements.  -> the reference of the pinned case."""
    ulp = 2.0 ** -6 if c.dtype == "bf16" else 2.0 ** -21
    for _ in range(40):
        r = ref_forward(c)
        if not c.relu:
            return r
        with np.errstate(invalid="ignore"):
            bad = (np.abs(r.pre) < 4.0 * r.e_pre) & (r.e_pre > 0)
        if not bad.any():
            return r
        # an exact 0 (two equal rows at M = 2) moves up in even rows, down in odd ones
        alt = np.where(np.arange(c.M)[:, None] % 2 == 0, 1.0, -1.0)
        sign = np.where(r.pre > 0, 1.0, np.where(r.pre < 0, -1.0, alt))
        if c.res is not None:
            step = np.maximum(8.0 * r.e_pre, ulp * np.abs(c.res) + 8 * SUB[c.dtype])
            c.res = np.where(bad, to_dtype(c.res + sign * step, c.dtype), c.res)
        else:
            a = np.broadcast_to(r.invstd * (1.0 if c.gamma is None else c.gamma), r.pre.shape)
            assert (a[bad] != 0).all(), "a zero-gain channel cannot be pinned through x"
            with np.errstate(divide="ignore", invalid="ignore"):
                step = np.maximum(8.0 * r.e_pre / np.abs(a), ulp * np.abs(c.x) + 8 * SUB[c.dtype])
            c.x = np.where(bad, to_dtype(c.x + sign * np.sign(a) * step, c.dtype), c.x)
    raise AssertionError(f"{c.name}: ReLU decisions not pinned after 40 rounds")


def synth_y(rng, M, C, dtype):
    """the forward output a backward case is handed: zeros, -0.0, clearly
    positive values, and in rows 1 and M - 2 the smallest positive subnormal"""
    kind = rng.integers(0, 4, (M, C))
    y = np.where(kind >= 2, 0.1 + 2.0 * rng.random((M, C)), 0.0).astype(F32)
    y = np.where(kind == 1, F32(-0.0), y)
    y = to_dtype(y, dtype)
    y = np.where(kind == 1, F32(-0.0), y).astype(F32)
    for row in {min(1, M - 1), max(M - 2, 0)}:
        y[row, ::2] = F32(SUB[dtype])
    return y


def _draw_backward(c, rng, mean=0.3, std=1.7):
    M, C = c.M, c.C
    c.dy = to_dtype(rng.standard_normal((M, C)), c.dtype)
    c.y = synth_y(rng, M, C, c.dtype)
    # near the statistics of x, but not equal to them
    c.bmean = (mean + 0.1 * std * rng.standard_normal(C)).astype(F32)
    c.binvstd = ((0.8 + 0.4 * rng.random(C)) / std).astype(F32)
    c.want_dres, c.want_dwb = c.bflags


def backward_args(c):
    return (c.dy, c.x, c.y if c.relu else None, c.gamma, c.bmean, c.binvstd, c.relu)


def ref_backward(c, model="kernel"):
    return backward(c.dy, c.x, c.y, c.gamma, c.bmean, c.binvstd, c.relu, dtype=c.dtype, model=model)


def _new(name, family, shape, dtype, k):
    N, C, H, W = shape
    return NS(name=f"{name}[{dtype}]", family=family, shape=shape, M=N * H * W, C=C, dtype=dtype,
              flags=FWD_FLAGS[k % len(FWD_FLAGS)], bflags=BWD_FLAGS[k % len(BWD_FLAGS)])


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def build_case(name, dtype="f32"):
    """The named case with every ReLU decision pinned.  Names: SHAPE_NAMES,
    EVAL_NAMES, OFFSET_NAMES (fp32), SYNTH_NAMES."""
    rng = np.random.default_rng(_seed(name))
    if name in SHAPE_NAMES:
        k = SHAPE_NAMES.index(name)
        family, _, shape = SHAPE_SPECS[k]
        c = _new(name, family, shape, dtype, k)
        if family == "stride":                 # a residual: one pinning round, not several
            c.flags, c.bflags = FWD_FLAGS[0], BWD_FLAGS[0]
        _draw_forward(c, rng)
        _draw_backward(c, rng)
    elif name in EVAL_NAMES:
        k = EVAL_NAMES.index(name)
        Cc, M = (int(p[1:]) for p in name.split("-")[1:])
        c = _new(name, "eval", (1, Cc, 1, M), dtype, k)
        c.flags = ((True, True, True, True, 0.1), (False, True, False, True, 0.1),
                   (True, False, True, True, 0.1))[k]
        _draw_forward(c, rng)
        _draw_backward(c, rng)
        c.training = False
    elif name in OFFSET_NAMES:
        assert dtype == "f32"
        c = _offset_case(name, rng)
    elif name in SYNTH_NAMES:
        c = _synth_case(name, dtype, rng)
    else:
        raise KeyError(name)
    c.ref = pin_relu(c)
    return c


def _offset_case(name, rng):
    """M = 9600, C = 8, fp32.  Channels 0-3: |mean - shift| / std = 0, 10, 100,
    1000 at std 1; 4: ratio 1000 at std 0.01; 5: ratio -100 at std 2; 6: exactly
    constant; 7: constant up to one ulp.  ``rm0``: running_mean = 0; ``null``: no
    running statistics; ``settled``: running_mean = the batch mean rounded to fp32."""
    c = _new(name, "offset", (2, 8, 60, 80), "f32", 0)
    M = c.M
    mean = np.array([0.0, 10.0, 100.0, 1000.0, 10.0, -200.0, 3.7, 3.7])
    std = np.array([1.0, 1.0, 1.0, 1.0, 0.01, 2.0, 0.0, 0.0])
    x = (rng.standard_normal((M, 8)) * std + mean).astype(F32)
    x[:, 0] -= x[:, 0].astype(F64).mean().astype(F32)
    x[:, 7] = np.where(rng.random(M) < 0.5, F32(3.7), np.nextafter(F32(3.7), F32(4)))
    c.x = x
    c.res = to_dtype(rng.standard_normal((M, 8)), "f32")
    c.gamma = (0.5 + rng.random(8)).astype(F32)
    c.beta = (rng.random(8) - 0.5).astype(F32)
    c.momentum, c.eps, c.relu, c.training = 0.1, 1e-5, True, True
    c.flags = (True, True, True, name != "offset-null", 0.1)
    if name == "offset-null":
        c.running_mean = c.running_var = None
    else:
        c.running_mean = np.zeros(8, F32) if name == "offset-rm0" else x.astype(F64).mean(0).astype(F32)
        c.running_var = np.ones(8, F32)
    c.ratio = np.array([0.0, 10.0, 100.0, 1000.0, 1000.0, 100.0, np.inf, np.inf])
    _draw_backward(c, rng)
    return c


def _synth_case(name, dtype, rng):
    """Backward on synthetic inputs, M = 1100, C = 8 (tq = 2, three row
    workgroups of 512 rows, 128 rows per iteration): ``mean1000``: x = 1000 + N(0, 1),
    mean / invstd to match; ``corr``: dy = 2 xhat + 0.05 noise; ``orth``: dy made
    orthogonal to 1 and to xhat over the batch before rounding."""
    c = _new(name, "synth", (1, 8, 1, 1100), dtype, 0)
    big = name == "synth-mean1000"
    c.flags = (True, True, True, True, 0.1)
    _draw_forward(c, rng, mean=1000.0 if big else 0.3, std=1.0 if big else 1.7)
    _draw_backward(c, rng, mean=1000.0 if big else 0.3, std=1.0 if big else 1.7)
    c.bflags = (True, True)
    c.want_dres, c.want_dwb = c.bflags
    xh = (c.x.astype(F64) - c.bmean) * c.binvstd
    if name == "synth-corr":
        c.dy = to_dtype(2.0 * xh + 0.05 * rng.standard_normal(xh.shape), dtype)
        c.relu = False
    elif name == "synth-orth":
        d = rng.standard_normal(xh.shape)
        d -= d.mean(0)
        xc = xh - xh.mean(0)
        d -= xc * ((d * xc).sum(0) / (xc * xc).sum(0))
        c.dy = to_dtype(d, dtype)
        c.relu = False
    return c


def with_nan(c, row, ch, value=np.nan):
    """a copy of the pinned case with x[row, ch] = value"""
    d = NS(**vars(c))
    d.x = c.x.copy()
    d.x[row, ch] = value
    d.name = c.name + "+nonfinite"
    d.nan_at = (row, ch)
    return d
