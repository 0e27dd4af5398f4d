"""numpy restatement of the MARCHED compositing entry points (include/ucsa_hip.h:
``ucsa_composite_rays_train_fwd/bwd``, ``ucsa_composite_rays``,
``ucsa_march_segment_composite``, ``ucsa_march_segment_shade{,_f16,_h2}``,
``ucsa_march_train_fwd/bwd``): the float64 yardstick of
tests/test_march_reference_cpu.py and tests/test_gpu_march_reference.py (test
infrastructure: plain numpy, no torch op, no GPU, no HIP library).

It is stated from ``oracle/raymarch.c`` / ``oracle/raymarch.py`` and the
contracts in the header; the nets, their backward, the comparison and the gate
pinning are those of tests/shade_numpy.py and are not restated.  It knows
nothing of waves, 64-sample trips, slot tables or carries: spans are gathered
into one padded row per ray ([n, K], K the longest span), one row per sample,
one sum per ray.

Bounds (``e_*``, per element, ABSOLUTE: behind an opaque sample the relative
error of 1 - alpha is unbounded) come from running error analysis, u = 2^-24:

  x     = sigma scale delta0           two products: 2 u x
  ex    = __expf(-x)                   ex (2^-22 + x u) (``_exp_rel``) + the
                                       argument's 2 u x ex + 2^-126 (the
                                       hardware exponential flushes denormals);
                                       x = 0 gives exactly 1 on both sides
  alpha = 1 - ex                       + u alpha
  fac   = 1 - alpha                    + u fac (covers a kernel that multiplies
                                       ex itself)
  T     ``product`` form: T_{i+1} = T_i fac_i, e_T fac + T e_fac + u T_{i+1},
        in any association (a scan tree and its carries): + 8 u T;
        ``sum`` form (``ucsa_composite_rays``: T_i = 1 - ws_i with ws the
        running fp32 sum): e_ws_i + u T_i; ws' = ws (1 - alpha) + alpha, so
        e_ws' = e_ws fac + e_alpha T + u (alpha T + w + ws')
  w     = alpha T                      e_alpha T + alpha e_T + u w
  t     = t0 + sum delta1              (k + 8) u (|t0| + sum |delta1|), any order
  a K-term sum of products w v added to a running value ``old``, in any order:
        sum (e_w |v| + w e_v) + (K + 2) u (|old| + sum |w v|).

Threshold decisions are NOT in the tolerance: the case builders place every
stop by construction (one sample takes T from >= 1e-2 to <= 1e-6), redraw the
sigma of a sample whose weight lies within its bound of ``w_min`` and the h row
of a sample with a hidden pre-activation within its bound of zero, and assert
that at most 5 % of a case was redrawn and that nothing is left undecided.

``dt=F32`` evaluates the same formulas in fp32 with sequential sums;
``mutant`` names one deliberate mistake (``MUTANTS``).
"""
import math
from types import SimpleNamespace as NS

import numpy as np

from tests import shade_numpy as sn
from tests.shade_numpy import (F32, F64, FP32, H2, LO, HI, REDRAW_CAP, U, F16M,
                               RedrawCap, _exp_rel, _np, compare, shade_backward,
                               shade_forward, split_nets)

THR = float(F32(1e-4))            # the stop threshold as the kernels hold it
FLUSH = 2.0 ** -126               # a hardware exponential below this is 0
MAX_SPAN = 1024                   # longest span the marched training composites
RPW_MAX = 128                     # MARCH_RPW_MAX of composite.hip
CMP_WAVES = 12                    # waves per workgroup of the fused kernels

MUTANTS = ("stop_before_take", "never_stop", "carry_lost_64", "t_from_zero",
           "depth_unmasked", "ws_masked", "keep_span_ending_at_M", "sem_attached",
           "alpha_from_delta1", "scale_ignored", "finished_ignores_cap",
           "overwrite_not_add", "suffix_inclusive", "depth_grad_dropped",
           "keep_span_1025")

a64 = lambda v: np.abs(np.asarray(v, F64))


# ---------------------------------------------------------------------------
# spans <-> padded rows
# ---------------------------------------------------------------------------
def pad_spans(off, cnt):
    """-> flat row index [n, K] (clamped inside the span or to 0) and the
    validity mask of every padded element, K = the longest span."""
    off, cnt = np.asarray(off, np.int64), np.asarray(cnt, np.int64)
    K = int(cnt.max()) if cnt.size else 0
    k = np.arange(K)[None, :]
    valid = k < cnt[:, None]
    idx = np.where(valid, off[:, None] + k, 0)
    return idx, valid


def _gather(a, idx, valid, dt):
    a = np.asarray(a, dt)
    if a.shape[0] == 0:
        return np.zeros(idx.shape + a.shape[1:], dt)
    g = a[idx]
    g[~valid] = 0
    return g


# ---------------------------------------------------------------------------
# weights of a batch of spans
# ---------------------------------------------------------------------------
def span_weights(sigma, deltas, T0=1.0, t0=0.0, sigma_scale=1.0, stop=False, w_min=0.0,
                 valid=None, ws0=None, form="product", dt=F64, mutant=()):
    """sigma [n, K], deltas [n, K, 2] (a single span may be given as [K], [K, 2]),
    T0 / t0 scalars or [n]; ``valid`` marks the real samples of a padded row.
      alpha = 1 - exp(-sigma scale delta0)
      T     = exclusive product from T0 (``ws0`` given: T0 = 1 - ws0; with
              form="sum" T_i = 1 - (ws0 + sum_{j<i} w_j), the recurrence of
              oracle/raymarch.c ``orc_composite_rays``)
      w     = alpha T,   t = t0 + cumsum(delta1)
      used  (``stop``): no EARLIER sample of the ray saw incoming T <= 1e-4f --
            the sample that sees it is still taken (raymarching.cu:693-706)
      keep  = used & (w > w_min)
    -> alpha, T (incoming, [n, K]), T_next (after the sample), w, t, used, keep,
    stopped [n] (a used sample saw T <= 1e-4f), their bounds e_*, and
    near_T / near_w: the decisions within their bound of the threshold."""
    one = np.ndim(sigma) == 1
    sigma = np.asarray(sigma, dt).reshape((1, -1) if one else np.shape(sigma))
    n, K = sigma.shape
    deltas = np.asarray(deltas, dt).reshape(n, K, 2)
    valid = np.ones((n, K), bool) if valid is None else np.asarray(valid, bool).reshape(n, K)
    scale = dt(1.0) if "scale_ignored" in mutant else dt(sigma_scale)
    d0 = deltas[:, :, 1] if "alpha_from_delta1" in mutant else deltas[:, :, 0]
    x = np.where(valid, sigma * scale * d0, dt(0))
    with np.errstate(under="ignore", over="ignore"):
        ex = np.exp(-x)
    alpha = dt(1.0) - ex
    fac = dt(1.0) - alpha
    x64, ex64, al64, fac64 = (np.asarray(v, F64) for v in (x, ex, alpha, fac))
    e_ex = np.where(x64 == 0, 0.0, ex64 * (_exp_rel(x64) + 2.0 * U * np.abs(x64)) + FLUSH)
    e_alpha = e_ex + U * np.abs(al64)
    e_fac = np.where(x64 == 0, 0.0, e_alpha + U * fac64)
    if ws0 is not None:
        ws0 = np.broadcast_to(np.asarray(ws0, dt), (n,))
        T0v, e_T0 = dt(1.0) - ws0, U * a64(dt(1.0) - ws0)
    else:
        T0v, e_T0 = np.broadcast_to(np.asarray(T0, dt), (n,)), np.zeros(n)
    T = np.empty((n, K + 1), dt)
    e_T = np.zeros((n, K + 1))
    w = np.zeros((n, K), dt)
    e_w = np.zeros((n, K))
    T[:, 0], e_T[:, 0] = T0v, e_T0
    if form == "product":
        for i in range(K):
            if "carry_lost_64" in mutant and i and i % 64 == 0:
                T[:, i] = T0v
            T[:, i + 1] = T[:, i] * fac[:, i]
            T64 = np.asarray(T[:, i:i + 2], F64)
            e_T[:, i + 1] = np.where(x64[:, i] == 0, e_T[:, i],
                                     e_T[:, i] * fac64[:, i] + T64[:, 0] * e_fac[:, i] + U * T64[:, 1])
        e_T[:, 1:] += 8.0 * U * a64(T[:, 1:])
        w = alpha * T[:, :K]
        e_w = e_alpha * a64(T[:, :K]) + np.abs(al64) * e_T[:, :K] + U * a64(w)
    else:
        assert ws0 is not None and form == "sum"
        run, e_run = ws0.copy(), np.zeros(n)
        for i in range(K):
            if "carry_lost_64" in mutant and i and i % 64 == 0:
                run = ws0.copy()
            T[:, i] = dt(1.0) - run
            e_T[:, i] = e_run + U * a64(T[:, i])
            w[:, i] = alpha[:, i] * T[:, i]
            e_w[:, i] = e_alpha[:, i] * a64(T[:, i]) + np.abs(al64[:, i]) * e_T[:, i] + U * a64(w[:, i])
            run = run + w[:, i]
            # ws' = ws (1 - alpha) + alpha: an error of ws CONTRACTS by 1 - alpha
            e_run = (e_run * fac64[:, i] + e_alpha[:, i] * a64(T[:, i])
                     + U * (np.abs(al64[:, i]) * a64(T[:, i]) + a64(w[:, i]) + a64(run)))
        T[:, K] = dt(1.0) - run
        e_T[:, K] = e_run + U * a64(T[:, K])
    e_w = np.where(al64 == 0, 0.0, e_w)
    Tin, e_Tin = T[:, :K], e_T[:, :K]
    hit = valid & (Tin <= dt(THR))
    if not stop or "never_stop" in mutant:
        used = valid.copy()
        stopped = np.zeros(n, bool)
    else:
        seen = np.logical_or.accumulate(hit, 1) if K else hit
        if "stop_before_take" in mutant:
            used = valid & ~seen
        else:
            used = valid & ~np.concatenate([np.zeros((n, 1), bool), seen[:, :-1]], 1)
        stopped = hit.any(1)
    w = np.where(used, w, dt(0))
    e_w = np.where(used, e_w, 0.0)
    t0v = np.broadcast_to(np.asarray(dt(0) if "t_from_zero" in mutant else t0, dt), (n,))
    d1 = np.where(valid, deltas[:, :, 1], dt(0))
    t = np.empty((n, K), dt)
    acc = t0v.copy()
    for i in range(K):
        acc = acc + d1[:, i]
        t[:, i] = acc
    A_t = a64(t0v)[:, None] + np.cumsum(a64(d1), 1)
    e_t = (np.arange(1, K + 1)[None, :] + 8.0) * U * A_t
    wm = dt(F32(w_min))
    keep = used & (w > wm)
    r = NS(n=n, K=K, valid=valid, x=x, alpha=alpha, e_alpha=e_alpha, T=Tin, e_T=e_Tin,
           T_next=T[:, 1:], e_T_next=e_T[:, 1:], w=w, e_w=e_w, t=t, e_t=e_t, used=used,
           keep=keep, stopped=stopped, hit=hit)
    r.near_T = valid & (np.abs(np.asarray(Tin, F64) - THR) <= e_Tin) if stop else np.zeros((n, K), bool)
    r.near_w = (used & (np.abs(np.asarray(w, F64) - float(wm)) <= e_w)) if w_min > 0 else np.zeros((n, K), bool)
    return r


def _acc(w, e_w, val, e_val, old, dt, mutant=()):
    """old + sum_k w_k val_k per ray, in any order.  w [n, K], val [n, K, D]."""
    term = w[:, :, None] * val
    n, K, D = term.shape
    start = np.zeros((n, D), dt) if (old is None or "overwrite_not_add" in mutant) else np.asarray(old, dt).reshape(n, D)
    if dt is F64:
        out = start + term.sum(1)
    else:
        out = start.copy()
        for k in range(K):
            out = out + term[:, k]
    A = a64(start) + a64(term).sum(1)
    E = (e_w[:, :, None] * a64(val) + a64(w)[:, :, None] * e_val).sum(1)
    cnt = (np.asarray(w, F64) != 0).sum(1)[:, None]
    return out, E + (cnt + 2.0) * U * A


def _scatter_rows(n, K, D, rows, cols, v, dt):
    out = np.zeros((n, K, D), dt)
    out[rows, cols] = v
    return out


# ---------------------------------------------------------------------------
# ucsa_composite_rays_train_fwd / _bwd
# ---------------------------------------------------------------------------
def _train_rows(rays, M, mutant, limit=None):
    rays = np.asarray(rays, np.int64).reshape(-1, 3)
    idx, off, cnt = rays[:, 0], rays[:, 1], rays[:, 2].copy()
    drop = (off + cnt > M) if "keep_span_ending_at_M" in mutant else (off + cnt >= M)
    if limit is not None:
        drop |= cnt > (limit + 1 if "keep_span_1025" in mutant else limit)
    cnt[drop] = 0
    return idx, off, cnt


def composite_train_forward(sigmas, rgbs, local_sem, deltas, rays, M, dt=F64, mutant=()):
    """rays [N, 3] = (ray id, first row, count), rows in any order; outputs by
    ray id.  Empty rays and rays with first + count >= M give zeros.
    depth = sum w t with t = cumsum(delta1) from 0 (no near, no norm)."""
    idx, off, cnt = _train_rows(rays, M, mutant)
    N = len(idx)
    pi, valid = pad_spans(off, cnt)
    sw = span_weights(_gather(sigmas, pi, valid, dt), _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt),
                      valid=valid, dt=dt, mutant=mutant)
    r = NS(sw=sw, idx=idx, off=off, cnt=cnt, pi=pi, valid=valid, N=N)
    z = np.zeros(sw.w.shape + (1,))
    out = {}
    out["weights_sum"] = _acc(sw.w, sw.e_w, np.ones(sw.w.shape + (1,), dt), z, None, dt)
    out["depth"] = _acc(sw.w, sw.e_w, sw.t[:, :, None], sw.e_t[:, :, None], None, dt)
    rgb = _gather(np.asarray(rgbs).reshape(-1, 3), pi, valid, dt)
    out["image"] = _acc(sw.w, sw.e_w, rgb, np.zeros(rgb.shape), None, dt)
    n_sem = 0 if local_sem is None else np.asarray(local_sem).shape[-1]
    if n_sem:
        ls = _gather(np.asarray(local_sem).reshape(-1, n_sem), pi, valid, dt)
        out["semantics"] = _acc(sw.w, sw.e_w, ls, np.zeros(ls.shape), None, dt)
    for k, (v, e) in out.items():
        full, efull = np.zeros((N,) + v.shape[1:], dt), np.zeros((N,) + v.shape[1:])
        full[idx], efull[idx] = v, e
        if k in ("weights_sum", "depth"):
            full, efull = full[:, 0], efull[:, 0]
        setattr(r, k, full)
        setattr(r, "e_" + k, efull)
    r.semantics = getattr(r, "semantics", None)
    return r


def composite_train_backward(grad_ws, grad_image, grad_sem, sigmas, rgbs, deltas, rays, M,
                             dt=F64, mutant=()):
    """The derivative of ``composite_train_forward`` wrt sigmas, rgbs and
    local_sem for upstream grad_ws [N], grad_image [N, 3], grad_sem [N, n_sem]
    (no depth gradient; the semantic weights are detached):
      grad_rgbs_m  = grad_image w_m,   grad_local_sem_m = grad_sem w_m
      grad_sigma_m = delta0_m ( sum_c grad_image_c (T_{m+1} rgb_mc - sum_{j>m} w_j rgb_jc)
                                + grad_ws (T_{m+1} - sum_{j>m} w_j) )
    evaluated from the inputs.  The kernel forms the suffix sums as (forward
    output) - (its own prefix scan): the forward output carries the forward
    bound, the prefix one bound per scan.  Rows of no composited ray stay 0."""
    idx, off, cnt = _train_rows(rays, M, mutant)
    pi, valid = pad_spans(off, cnt)
    dl = _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt)
    sw = span_weights(_gather(sigmas, pi, valid, dt), dl, valid=valid, dt=dt, mutant=mutant)
    n, K = sw.w.shape
    rgb = _gather(np.asarray(rgbs).reshape(-1, 3), pi, valid, dt)
    gi = np.asarray(grad_image, dt).reshape(-1, 3)[idx]
    gw = np.asarray(grad_ws, dt).reshape(-1)[idx]
    # channels: r, g, b and the constant 1 of weights_sum
    val = np.concatenate([rgb, valid[:, :, None].astype(dt)], 2)
    gch = np.concatenate([gi, gw[:, None]], 1)
    term = sw.w[:, :, None] * val
    if dt is F64:
        pre = np.cumsum(term, 1)
    else:
        pre = np.empty_like(term)
        acc = np.zeros((n, 4), dt)
        for k in range(K):
            acc = acc + term[:, k]
            pre[:, k] = acc
    tot = pre[:, -1:] if K else np.zeros((n, 1, 4), dt)
    A_pre = np.cumsum(a64(term), 1)
    E_pre = np.cumsum(sw.e_w[:, :, None] * a64(val), 1)
    kk = np.arange(1, K + 1)[None, :, None]
    e_pre = E_pre + (kk + 8.0) * U * A_pre
    e_tot = (E_pre[:, -1:] + (cnt[:, None, None] + 2.0) * U * A_pre[:, -1:]) if K else np.zeros((n, 1, 4))
    suf = tot - pre
    if "suffix_inclusive" in mutant:
        suf = suf + term
    e_suf = e_tot + e_pre + 2.0 * U * (a64(tot) + a64(pre))
    Tn, e_Tn = sw.T_next[:, :, None], sw.e_T_next[:, :, None]
    tv = Tn * val
    inner = tv - suf
    e_inner = e_Tn * a64(val) + U * a64(tv) + e_suf + U * a64(inner)
    prod = gch[:, None, :] * inner
    s = prod.sum(2) if dt is F64 else ((prod[:, :, 0] + prod[:, :, 1]) + prod[:, :, 2]) + prod[:, :, 3]
    e_s = (a64(gch)[:, None, :] * e_inner).sum(2) + 6.0 * U * a64(prod).sum(2)
    gsig = dl[:, :, 0] * s
    e_gsig = a64(dl[:, :, 0]) * e_s + U * a64(gsig)
    if "sem_attached" in mutant and grad_sem is not None:
        gsig = gsig + dl[:, :, 0] * sw.T_next * np.asarray(grad_sem, dt)[idx].sum(1)[:, None]
    Mi = int(M)
    r = NS(sw=sw)

    def scatter(v, e, D):
        full, efull = np.zeros((Mi, D), dt), np.zeros((Mi, D))
        full[pi[valid]], efull[pi[valid]] = v[valid], e[valid]
        return full, efull

    g, e = scatter(gsig[:, :, None], e_gsig[:, :, None], 1)
    r.grad_sigmas, r.e_grad_sigmas = g[:, 0], e[:, 0]
    grgb = gi[:, None, :] * sw.w[:, :, None]
    r.grad_rgbs, r.e_grad_rgbs = scatter(grgb, a64(gi)[:, None, :] * sw.e_w[:, :, None] + U * a64(grgb), 3)
    r.grad_local_sem = r.e_grad_local_sem = None
    if grad_sem is not None:
        gs = np.asarray(grad_sem, dt)[idx]
        gls = gs[:, None, :] * sw.w[:, :, None]
        r.grad_local_sem, r.e_grad_local_sem = scatter(
            gls, a64(gs)[:, None, :] * sw.e_w[:, :, None] + U * a64(gls), gs.shape[1])
    return r


# ---------------------------------------------------------------------------
# the in-place updates: ucsa_composite_rays, ucsa_march_segment_composite,
# ucsa_march_segment_shade*
# ---------------------------------------------------------------------------
def _update(sw, ray, running, vals, dt, mutant, shaded=False):
    """running: dict name -> array by ray id (copied); vals: name -> (val, e_val)
    [n, K, D].  With ``shaded`` the image / semantics / depth sums run over the
    kept samples and weights_sum over the used ones."""
    out = {}
    n, K = sw.w.shape
    keep = sw.keep if shaded else sw.used
    wk, e_wk = np.where(keep, sw.w, dt(0)), np.where(keep, sw.e_w, 0.0)
    for name, (val, e_val) in vals.items():
        w, e_w = wk, e_wk
        if name == "weights_sum" and "ws_masked" not in mutant:
            w, e_w = sw.w, sw.e_w
        if name == "depth" and "depth_unmasked" in mutant:
            w, e_w = sw.w, sw.e_w
        full = np.array(running[name], dt, copy=True)
        flat = full.reshape(full.shape[0], -1)
        efull = np.zeros(flat.shape)
        v, e = _acc(w, e_w, val, e_val, flat[ray], dt, mutant)
        flat[ray], efull[ray] = v, e
        out[name] = (full, efull.reshape(full.shape))
    return out


def _finish(r, out):
    for k, (v, e) in out.items():
        setattr(r, k, v)
        setattr(r, "e_" + k, e)
    return r


def composite_rays_update(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, local_sem, deltas,
                          weights_sum, depth, image, semantics, dt=F64, mutant=()):
    """oracle/raymarch.c ``orc_composite_rays``: slot n < n_alive owns rows
    [n n_step, (n + 1) n_step); a row with delta0 == 0 ends the ray; sums are
    accumulated in place by ray id; rays_t[n] = -1 when the ray ended (zero
    delta, or a taken sample saw T <= 1e-4), else the parameter after its last
    sample.  Slots >= n_alive and rays of no slot keep their values."""
    ra = np.asarray(rays_alive, np.int64)[:n_alive]
    dl_all = np.asarray(deltas).reshape(-1, 2)
    d0 = np.asarray(dl_all[:n_alive * n_step, 0]).reshape(n_alive, n_step)
    zero = d0 == 0
    cnt = np.where(zero.any(1), zero.argmax(1), n_step)
    off = np.arange(n_alive) * n_step
    pi, valid = pad_spans(off, cnt)
    ws_in = np.asarray(weights_sum, dt).reshape(-1)
    t_in = np.asarray(rays_t, dt).reshape(-1)
    sw = span_weights(_gather(sigmas, pi, valid, dt), _gather(dl_all, pi, valid, dt), t0=t_in[:n_alive],
                      stop=True, valid=valid, ws0=ws_in[ra], form="sum", dt=dt, mutant=mutant)
    r = NS(sw=sw, cnt=cnt, ra=ra)
    vals = _plain_vals(sw, pi, valid, rgbs, local_sem, dt)
    running = dict(weights_sum=weights_sum, depth=depth, image=image, semantics=semantics)
    _finish(r, _update(sw, ra, running, vals, dt, mutant))
    full = (cnt == n_step) & ~sw.stopped
    _set_rays_t(r, sw, t_in, n_alive, full, cnt, dt)
    return r


def _plain_vals(sw, pi, valid, rgbs, local_sem, dt):
    rgb = _gather(np.asarray(rgbs).reshape(-1, 3), pi, valid, dt)
    vals = dict(weights_sum=(np.ones(sw.w.shape + (1,), dt), np.zeros(sw.w.shape + (1,))),
                depth=(sw.t[:, :, None], sw.e_t[:, :, None]), image=(rgb, np.zeros(rgb.shape)))
    if local_sem is not None:
        n_sem = np.asarray(local_sem).shape[-1]
        ls = _gather(np.asarray(local_sem).reshape(-1, n_sem), pi, valid, dt)
        vals["semantics"] = (ls, np.zeros(ls.shape))
    return vals


def _set_rays_t(r, sw, t_in, n_alive, goes_on, cnt, dt):
    r.rays_t, r.e_rays_t = t_in.copy(), np.zeros(t_in.shape)
    last = np.maximum(cnt, 1) - 1
    rows = np.arange(n_alive)
    t_last = np.where(cnt > 0, sw.t[rows, last] if sw.K else t_in[:n_alive], t_in[:n_alive])
    e_last = np.where(cnt > 0, sw.e_t[rows, last] if sw.K else 0.0, 0.0)
    r.rays_t[:n_alive] = np.where(goes_on, t_last, dt(-1.0))
    r.e_rays_t[:n_alive] = np.where(goes_on, e_last, 0.0)
    r.finished = ~goes_on


def segment_composite(n_alive, cap, rays_alive, rays_t, span, sigmas, sigma_scale, rgbs, local_sem,
                      deltas, weights_sum, depth, image, semantics, dt=F64, mutant=()):
    """``ucsa_march_segment_composite``: slot n < n_alive composites rows
    span[n] = (first, count) from T0 = 1 - weights_sum[ray], t0 = rays_t[n], with
    the stop rule; rays_t[n] = -1 iff the ray stopped or count < cap."""
    ra = np.asarray(rays_alive, np.int64)[:n_alive]
    sp = np.asarray(span, np.int64).reshape(-1, 2)[:n_alive]
    pi, valid = pad_spans(sp[:, 0], sp[:, 1])
    ws_in = np.asarray(weights_sum, dt).reshape(-1)
    t_in = np.asarray(rays_t, dt).reshape(-1)
    sw = span_weights(_gather(sigmas, pi, valid, dt), _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt),
                      t0=t_in[:n_alive], sigma_scale=sigma_scale, stop=True, valid=valid, ws0=ws_in[ra],
                      dt=dt, mutant=mutant)
    r = NS(sw=sw, ra=ra, cnt=sp[:, 1])
    vals = _plain_vals(sw, pi, valid, rgbs, local_sem, dt)
    running = dict(weights_sum=weights_sum, depth=depth, image=image, semantics=semantics)
    _finish(r, _update(sw, ra, running, vals, dt, mutant))
    goes_on = ~sw.stopped if "finished_ignores_cap" in mutant else ~sw.stopped & (sp[:, 1] >= cap)
    _set_rays_t(r, sw, t_in, n_alive, goes_on, sp[:, 1], dt)
    return r


def _shaded_vals(sw, ray, pi, rays_d, h, nets, C, mode, dt, mutant):
    """the nets on the kept samples only -> vals of ``_update`` and the flat
    shading record (rows, cols of the kept samples)."""
    rows, cols = np.nonzero(sw.keep)
    hh = np.asarray(_np(h, F32)).reshape(-1, 16)
    dirs = np.asarray(_np(rays_d, F32)).reshape(-1, 3)
    f = shade_forward(dirs[ray[rows]], hh[pi[rows, cols], 1:], nets, C, mode, dt)
    n, K = sw.w.shape
    put = lambda v, D, t: _scatter_rows(n, K, D, rows, cols, v, t)
    vals = dict(weights_sum=(np.ones((n, K, 1), dt), np.zeros((n, K, 1))),
                depth=(sw.t[:, :, None], sw.e_t[:, :, None]),
                image=(put(f.rgb, 3, dt), put(f.e_rgb, 3, F64)),
                semantics=(put(f.p[:, :C], C, dt), put(f.e_p[:, :C], C, F64)))
    return vals, f, rows, cols


def segment_shade(mode, n_alive, cap, rays_alive, rays_t, span, rays_d, sigmas, sigma_scale, h,
                  deltas, color_params, sem_params, C, w_min, weights_sum, depth, image, semantics,
                  dt=F64, mutant=()):
    """``ucsa_march_segment_shade{,_f16,_h2}`` (mode FP32 / F16M() / H2): the
    weights of ``segment_composite``; the colour and semantics nets run on the
    samples with w > w_min only (h [M, 16] raw sigma-net rows, rays_d by ray
    id); image, semantics and depth are summed over those, weights_sum over
    every used sample; everything is added in place."""
    ra = np.asarray(rays_alive, np.int64)[:n_alive]
    sp = np.asarray(span, np.int64).reshape(-1, 2)[:n_alive]
    pi, valid = pad_spans(sp[:, 0], sp[:, 1])
    ws_in = np.asarray(weights_sum, dt).reshape(-1)
    t_in = np.asarray(rays_t, dt).reshape(-1)
    sw = span_weights(_gather(sigmas, pi, valid, dt), _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt),
                      t0=t_in[:n_alive], sigma_scale=sigma_scale, stop=True, w_min=w_min, valid=valid,
                      ws0=ws_in[ra], dt=dt, mutant=mutant)
    nets = split_nets(color_params, sem_params, C, mode, dt)
    vals, f, rows, cols = _shaded_vals(sw, ra, pi, rays_d, h, nets, C, mode, dt, mutant)
    r = NS(sw=sw, ra=ra, cnt=sp[:, 1], f=f, pi=pi)
    running = dict(weights_sum=weights_sum, depth=depth, image=image, semantics=semantics)
    _finish(r, _update(sw, ra, running, vals, dt, mutant, shaded=True))
    goes_on = ~sw.stopped if "finished_ignores_cap" in mutant else ~sw.stopped & (sp[:, 1] >= cap)
    _set_rays_t(r, sw, t_in, n_alive, goes_on, sp[:, 1], dt)
    return r


# ---------------------------------------------------------------------------
# ucsa_march_train_fwd / _bwd
# ---------------------------------------------------------------------------
def march_train_forward(rays, M, nears, rays_d, sigmas, sigma_scale, h, deltas, color_params,
                        sem_params, C, w_min, mode=FP32, dt=F64, mutant=()):
    """No stop; t measured from nears[ray]; spans reaching M or longer than 1024
    samples are dropped (zero outputs).  -> weights_sum, depth (the raw
    sum w t over the kept samples), image, semantics by ray id, w_out, t_out [M]
    (zero outside the composited spans)."""
    idx, off, cnt = _train_rows(rays, M, mutant, limit=MAX_SPAN)
    N = len(idx)
    pi, valid = pad_spans(off, cnt)
    t0 = np.asarray(nears, dt).reshape(-1)[idx]
    sw = span_weights(_gather(sigmas, pi, valid, dt), _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt),
                      t0=t0, sigma_scale=sigma_scale, w_min=w_min, valid=valid, dt=dt, mutant=mutant)
    nets = split_nets(color_params, sem_params, C, mode, dt)
    vals, f, rows, cols = _shaded_vals(sw, idx, pi, rays_d, h, nets, C, mode, dt, mutant)
    r = NS(sw=sw, idx=idx, f=f, pi=pi, valid=valid)
    running = dict(weights_sum=np.zeros(N, dt), depth=np.zeros(N, dt), image=np.zeros((N, 3), dt),
                   semantics=np.zeros((N, C), dt))
    _finish(r, _update(sw, idx, running, vals, dt, mutant, shaded=True))
    for name, v, e in (("w_out", sw.w, sw.e_w), ("t_out", sw.t, sw.e_t)):
        full, efull = np.zeros(int(M), dt), np.zeros(int(M))
        full[pi[valid]], efull[pi[valid]] = v[valid], e[valid]
        setattr(r, name, full)
        setattr(r, "e_" + name, efull)
    return r


def march_train_backward(rays, M, rays_d, norms, sigmas, sigma_scale, h, deltas, w_all, t_all,
                         color_params, sem_params, C, w_min, d_image, d_depth, d_sem, mode=FP32,
                         dt=F64, mutant=()):
    """Backward of ``march_train_forward`` for d_image [N, 3], d_depth [N] (wrt
    depth / norms[ray]) and d_sem [N, C]; w_all / t_all are the fp32 arrays the
    entry point receives (the mask is w_all > w_min on those numbers).
      G_m       = d_depth t_m / norm + d_image . rgb_m      (kept samples, else 0)
      d_sigma_m = delta0_m scale (G_m T_{m+1} - sum_{j>m} G_j w_j)
      d_h[m, 0] = d_sigma_m clamp(sigma_m, e^-15, e^15)     (trunc_exp backward)
      d_h[m, 1:] = the nets' gradient wrt the geo features (kept samples)
    -> G [M], d_h [M, 16], dW_color, dW_sem with bounds."""
    idx, off, cnt = _train_rows(rays, M, mutant, limit=MAX_SPAN)
    pi, valid = pad_spans(off, cnt)
    n, K = pi.shape
    sig = _gather(sigmas, pi, valid, dt)
    dl = _gather(np.asarray(deltas).reshape(-1, 2), pi, valid, dt)
    sw = span_weights(sig, dl, sigma_scale=sigma_scale, valid=valid, dt=dt, mutant=mutant)
    w32 = np.asarray(_np(w_all, F32)).reshape(-1)
    wv = _gather(w32, pi, valid, dt)
    tv = _gather(np.asarray(_np(t_all, F32)).reshape(-1), pi, valid, dt)
    keep = valid & (_gather(w32, pi, valid, F32) > F32(w_min))
    rows, cols = np.nonzero(keep)
    nets = split_nets(color_params, sem_params, C, mode, dt)
    hh = np.asarray(_np(h, F32)).reshape(-1, 16)
    dirs = np.asarray(_np(rays_d, F32)).reshape(-1, 3)
    ray = idx[rows]
    f = shade_forward(dirs[ray], hh[pi[rows, cols], 1:], nets, C, mode, dt)
    dd = np.asarray(_np(d_depth, F32)).reshape(-1)[ray]
    if "depth_grad_dropped" in mutant:
        dd = np.zeros_like(dd)
    smut = ("sem_not_detached",) if "sem_attached" in mutant else ()
    b = shade_backward(f, wv[rows, cols], np.asarray(_np(d_image, F32)).reshape(-1, 3)[ray], dd,
                       np.asarray(_np(d_sem, F32)).reshape(-1, C)[ray], tv[rows, cols],
                       np.asarray(_np(norms, F32)).reshape(-1)[ray], nets, C, mode, dt, smut)
    G, e_G = np.zeros((n, K), dt), np.zeros((n, K))
    G[rows, cols], e_G[rows, cols] = b.G, b.e_G
    q = G * wv
    e_q = e_G * a64(wv) + U * a64(q)
    if dt is F64:
        rev = np.cumsum(q[:, ::-1], 1)[:, ::-1]
    else:
        rev = np.empty_like(q)
        acc = np.zeros(n, dt)
        for k in range(K - 1, -1, -1):
            acc = acc + q[:, k]
            rev[:, k] = acc
    A_rev = np.cumsum(a64(q)[:, ::-1], 1)[:, ::-1]
    E_rev = np.cumsum(e_q[:, ::-1], 1)[:, ::-1]
    z1 = np.zeros((n, 1))
    if "suffix_inclusive" in mutant:
        suf, A_suf, E_suf = rev, A_rev, E_rev
    else:
        suf = np.concatenate([rev[:, 1:], z1.astype(dt)], 1)
        A_suf = np.concatenate([A_rev[:, 1:], z1], 1)
        E_suf = np.concatenate([E_rev[:, 1:], z1], 1)
    if "carry_lost_64" in mutant and K:
        # the reverse scan runs in passes of 64 from the far end of each span
        kk = cnt[:, None] - 1 - np.arange(K)[None, :]
        first = np.clip(cnt[:, None] - (kk // 64) * 64, 0, K)
        revx = np.concatenate([rev, z1.astype(dt)], 1)
        suf = np.where(valid, suf - np.take_along_axis(revx, first, 1), suf)
    e_suf = E_suf + (K / 64.0 + 8.0) * U * A_suf
    Tn, e_Tn = sw.T_next, sw.e_T_next
    t1 = G * Tn
    inner = t1 - suf
    e_inner = e_G * a64(Tn) + a64(G) * e_Tn + U * a64(t1) + e_suf + U * a64(inner)
    scale = dt(sigma_scale)
    m_ = dl[:, :, 0] * scale
    dsig = m_ * inner
    e_dsig = a64(m_) * e_inner + 2.0 * U * a64(dsig)
    c = np.clip(sig, dt(LO), dt(HI))
    dh0 = dsig * c
    e_dh0 = e_dsig * a64(c) + 3.0 * U * a64(dh0)
    Mi = max(int(M), 0)
    r = NS(sw=sw, f=f, b=b, keep=keep)
    r.G, r.e_G = np.zeros(Mi, dt), np.zeros(Mi)
    r.G[pi[valid]], r.e_G[pi[valid]] = G[valid], e_G[valid]
    r.d_h, r.e_d_h = np.zeros((Mi, 16), dt), np.zeros((Mi, 16))
    r.d_h[pi[valid], 0], r.e_d_h[pi[valid], 0] = dh0[valid], e_dh0[valid]
    flat = pi[rows, cols]
    r.d_h[flat, 1:], r.e_d_h[flat, 1:] = b.dgeo, b.e_dgeo
    r.dW_color, r.e_dW_color, r.dW_sem, r.e_dW_sem = b.dW_color, b.e_dW_color, b.dW_sem, b.e_dW_sem
    r.composited = np.zeros(Mi, bool)
    r.composited[pi[valid]] = True
    return r


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def compare_fields(got, ref, keys, what, where=""):
    """got: dict name -> array; every named field of ``ref`` within its bound."""
    worst = 0.0
    for k in keys:
        if got.get(k) is None or getattr(ref, k, None) is None:
            continue
        v = np.asarray(getattr(ref, k), F64)
        worst = max(worst, compare(np.asarray(_np(got[k], F64)).reshape(v.shape), v, getattr(ref, "e_" + k),
                                   f"{what} {k} @ {where}"))
    return worst


def passes(got, ref, keys, what="mutant"):
    """the comparison as a predicate (for the mutant table); leaves WORST alone"""
    saved = dict(sn.WORST)
    try:
        compare_fields(got, ref, keys, what)
        return True
    except sn.Mismatch:
        return False
    finally:
        sn.WORST.clear()
        sn.WORST.update(saved)


def as_got(ref, keys):
    return {k: getattr(ref, k) for k in keys if getattr(ref, k, None) is not None}


# ---------------------------------------------------------------------------
# cases of the reference-API kernels
# ---------------------------------------------------------------------------
SPAN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1024)
RAY_COUNTS = (1, 3, 4, 5, 257)
SEM_COUNTS = (0, 1, 63, 64, 65, 128, 129, 255, 256)
STOP_AT = (0, 62, 63, 64, 128, 129)     # in a 130-sample span: head, lanes 62 / 63 of a
                                        # trip, lane 0 of the next two trips, tail
TRAIN_KEYS = ("weights_sum", "depth", "image", "semantics")
TRAIN_BWD_KEYS = ("grad_sigmas", "grad_rgbs", "grad_local_sem")
UPDATE_KEYS = ("weights_sum", "depth", "image", "semantics", "rays_t")


def _samples(rng, counts, depth_total=3.0):
    """sigma / deltas of contiguous spans of the given lengths: optical depth
    ~depth_total per ray spread over its samples (so T stays above 1e-2 without
    a placed opaque sample), delta1 = delta0 plus an occasional skipped gap."""
    counts = np.asarray(counts, np.int64)
    M = int(counts.sum())
    ray = np.repeat(np.arange(len(counts)), counts)
    d0 = (0.004 + 0.02 * rng.random(M)).astype(F32)
    gap = np.where(rng.random(M) < 0.2, 0.05 * rng.random(M), 0.0)
    d1 = (d0 + gap).astype(F32)
    per = depth_total / np.maximum(counts[ray], 1)
    sigma = (per / d0 * (0.2 + 1.3 * rng.random(M))).astype(F32)
    return ray, sigma, np.stack([d0, d1], 1)


def _place(c, off, k, x):
    """sample k of the span at `off` gets optical depth x"""
    c.sigmas[off + k] = F32(x / (float(c.deltas[off + k, 0]) * c.sigma_scale))


def case_train(name, counts, n_sem, seed, drop_last=False, special=False):
    """ucsa_composite_rays_train_*: rays of the given lengths (0 = empty),
    contiguous spans, ray ids and row order both permuted.  The last non-empty
    span ends at M - 1 (kept) or, with ``drop_last``, at M (dropped).
    ``special``: ray 0 has an opaque sample (optical depth 200 > 88: the fp32
    exponential is exactly 0) at a third of its span, ray 1 a half-opaque one
    (30), ray 2 only sigma = 0 samples, and every 7th sample anywhere sigma = 0."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    N = len(counts)
    ray, sigma, deltas = _samples(rng, counts)
    total = int(counts.sum())
    M = total if drop_last else total + 1
    c = NS(name=name, N=N, M=M, n_sem=n_sem, sigma_scale=1.0)
    pad = M - total
    c.sigmas = np.concatenate([sigma, np.ones(pad, F32)])
    c.deltas = np.concatenate([deltas, np.full((pad, 2), 0.01, F32)])
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])
    if special:
        c.sigmas[::7] = 0
        nz = [i for i in range(N) if counts[i] >= 3]
        if len(nz) > 0:
            _place(c, off[nz[0]], counts[nz[0]] // 3, 200.0)
        if len(nz) > 1:
            _place(c, off[nz[1]], counts[nz[1]] // 2, 30.0)
        if len(nz) > 2:
            c.sigmas[off[nz[2]]:off[nz[2]] + counts[nz[2]]] = 0
    c.rgbs = rng.random((M, 3)).astype(F32)
    ls = rng.random((M, max(n_sem, 1))).astype(F32)
    c.local_sem = (ls / ls.sum(1, keepdims=True)).astype(F32) if n_sem else None
    ids = rng.permutation(N)
    rays = np.stack([ids, off, counts], 1).astype(np.int32)
    c.rays = np.ascontiguousarray(rays[rng.permutation(N)])
    c.dropped = c.rays[:, 1].astype(np.int64) + c.rays[:, 2] >= M
    c.g_ws = rng.standard_normal(N).astype(F32)
    c.g_img = rng.standard_normal((N, 3)).astype(F32)
    c.g_sem = rng.standard_normal((N, n_sem)).astype(F32) if n_sem else None
    c.redrawn = 0.0
    return c


def _mixed_counts(N, rng):
    """N rays over SPAN_LENGTHS (1024 once), empty rays first, in the middle and last"""
    if N == 1:
        return [65]
    pool = [v for v in SPAN_LENGTHS if v != 1024]
    cnt = [pool[i % len(pool)] for i in range(N)]
    cnt[0] = 0
    cnt[N // 2] = 0
    cnt[-1] = 0
    if N >= 4:
        cnt[1] = 1024
    return cnt


def train_case_specs():
    """name -> builder arguments of every ucsa_composite_rays_train_* case"""
    s = {}
    for L in SPAN_LENGTHS:
        s[f"len{L}"] = dict(counts=[L, 0, L], n_sem=6, seed=100 + L, special=L >= 63)
    for N in RAY_COUNTS:
        s[f"rays{N}"] = dict(counts=None, N=N, n_sem=3, seed=200 + N, special=True)
    for k in SEM_COUNTS:
        s[f"sem{k}"] = dict(counts=[5, 0, 70, 129, 0], n_sem=k, seed=300 + k, special=k in (0, 256))
    s["dropped"] = dict(counts=[0, 64, 3, 0, 130, 0], n_sem=5, seed=400, drop_last=True, special=True)
    return s


def build_train_case(name):
    a = dict(train_case_specs()[name])
    if a.get("counts") is None:
        a["counts"] = _mixed_counts(a.pop("N"), np.random.default_rng(a["seed"]))
    a.pop("N", None)
    return case_train(name, **a)


def train_refs(c, dt=F64, mutant=()):
    fw = composite_train_forward(c.sigmas, c.rgbs, c.local_sem, c.deltas, c.rays, c.M, dt, mutant)
    bw = composite_train_backward(c.g_ws, c.g_img, c.g_sem, c.sigmas, c.rgbs, c.deltas, c.rays, c.M,
                                  dt, mutant)
    return fw, bw


def case_update(name, counts, n_sem, seed, stops=(), head_stop=(), zero_delta=(), cap=None,
                sigma_scale=1.0, n_extra=2, second_round=True, tight_stop=()):
    """The in-place kernels (``ucsa_march_segment_composite`` directly;
    ``ucsa_composite_rays`` through ``as_steps``).  Slots in order, spans
    contiguous, ray ids permuted among N = slots + n_extra rays (the extra rays
    belong to no slot), running sums non-zero on entry (``second_round``),
    n_alive = slots - 1 < n_cap = slots: the last slot is not alive.
      stops      {slot: k}: sample k - 1 takes T from >= 1e-2 to <= 1e-6, so
                 sample k is the one that sees T <= 1e-4 (taken, the last)
      head_stop  slots whose ray enters with 1 - weights_sum <= 1e-6
      tight_stop slots whose sample 0 takes T to 8e-7, the nearest the rule above
                 allows, and whose sample 1 -- the one that sees it -- is opaque
                 with rgb = 64: in so short a span leaving it out shows
      zero_delta {slot: k}: row k has delta0 == 0 (composite_rays only)
    Every other decision is asserted to be clear of its bound by ``check_pinned``."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    ray, sigma, deltas = _samples(rng, counts, depth_total=2.0)
    M = int(counts.sum())
    c = NS(name=name, n_cap=n, n_alive=max(n - 1, 1) if n > 1 else 1, n_sem=n_sem, M=M,
           sigma_scale=float(sigma_scale), N=n + n_extra)
    c.sigmas = (sigma / F32(sigma_scale)).astype(F32)
    c.deltas = deltas
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    c.span = np.stack([off, counts], 1).astype(np.int32)
    c.cap = int(counts.max()) if cap is None else int(cap)
    for s, k in dict(stops).items():
        assert 1 <= k < counts[s]
        _place(c, off[s], k - 1, 16.0)
    c.zero_delta, c.stops = dict(zero_delta), dict(stops)
    c.rgbs = rng.random((M, 3)).astype(F32)
    ls = rng.random((M, max(n_sem, 1))).astype(F32)
    c.local_sem = (ls / ls.sum(1, keepdims=True)).astype(F32) if n_sem else None
    c.rays_alive = rng.permutation(c.N)[:n].astype(np.int32)
    c.rays_t = (0.3 + rng.random(n)).astype(F32)
    N = c.N
    if second_round:
        c.weights_sum = (0.5 * rng.random(N)).astype(F32)
        c.depth = rng.random(N).astype(F32)
        c.image = (0.5 * rng.random((N, 3))).astype(F32)
        c.semantics = (0.5 * rng.random((N, max(n_sem, 1)))).astype(F32)
    else:
        c.weights_sum, c.depth = np.zeros(N, F32), np.zeros(N, F32)
        c.image, c.semantics = np.zeros((N, 3), F32), np.zeros((N, max(n_sem, 1)), F32)
    if not n_sem:
        c.semantics = None
    for s in head_stop:
        c.weights_sum[c.rays_alive[s]] = F32(1.0 - 1e-6)
    for s in tight_stop:
        assert counts[s] >= 2
        T0 = 1.0 - float(c.weights_sum[c.rays_alive[s]])
        _place(c, off[s], 0, math.log(T0 / 8e-7))
        _place(c, off[s], 1, 16.0)
        c.rgbs[off[s] + 1] = 64.0
        c.stops[s] = 1
    c.redrawn = 0.0
    return c


def as_steps(c):
    """the same slots as the padded rows of ``ucsa_composite_rays``: n_step =
    the longest span (+ 1 when a zero-delta row is asked for past it), rows
    past a span zero (delta0 == 0 ends the ray), a placed zero-delta row cuts
    its span short -> (n_step, sigmas, rgbs, local_sem, deltas)"""
    cnt = c.span[:, 1].astype(np.int64)
    n_step = int(cnt.max())
    n = c.n_cap
    sig, dl = np.zeros((n, n_step), F32), np.zeros((n, n_step, 2), F32)
    rgb = np.zeros((n, n_step, 3), F32)
    ls = np.zeros((n, n_step, max(c.n_sem, 1)), F32)
    for s in range(n):
        o, k = int(c.span[s, 0]), int(cnt[s])
        sig[s, :k], dl[s, :k], rgb[s, :k] = c.sigmas[o:o + k] * F32(c.sigma_scale), c.deltas[o:o + k], c.rgbs[o:o + k]
        if c.n_sem:
            ls[s, :k] = c.local_sem[o:o + k]
    for s, k in c.zero_delta.items():
        dl[s, k, 0] = 0
    return (n_step, sig.reshape(-1), rgb.reshape(-1, 3), ls.reshape(n * n_step, -1) if c.n_sem else None,
            dl.reshape(-1, 2))


def update_case_specs():
    s = {}
    for L in SPAN_LENGTHS:
        s[f"len{L}"] = dict(counts=[L, 3, L, 2], n_sem=4, seed=500 + L,
                            stops=({0: L - 1} if L >= 63 else {}))   # a stop on the tail
    for k in STOP_AT:
        if k == 0:
            s["stop_head"] = dict(counts=[130, 130, 5, 1, 9], n_sem=3, seed=600, head_stop=(0, 3))
        else:
            s[f"stop{k}"] = dict(counts=[130, 7, 130, 9], n_sem=3, seed=600 + k, stops={0: k, 2: k},
                                 tight_stop=(1,))
    for N in RAY_COUNTS:
        cnt = [int(v) for v in np.random.default_rng(700 + N).integers(0, 9, N + 1)]
        cnt[0] = 0
        cnt[-1] = max(cnt[-1], 1)
        if N >= 3:
            cnt[N // 2] = 0
            cnt[-2] = 0
            cnt[1] = 70
        s[f"slots{N}"] = dict(counts=cnt, n_sem=2, seed=700 + N, cap=70)
    for k in SEM_COUNTS:
        s[f"sem{k}"] = dict(counts=[5, 0, 70, 129, 3], n_sem=k, seed=800 + k, stops={3: 64})
    s["scale"] = dict(counts=[40, 66, 3], n_sem=2, seed=900, sigma_scale=0.37, stops={1: 65})
    s["cap_above"] = dict(counts=[12, 12, 3, 12], n_sem=2, seed=901, cap=13)
    s["cap_equal"] = dict(counts=[12, 12, 3, 12], n_sem=2, seed=902, cap=12, stops={1: 11})
    s["first_round"] = dict(counts=[64, 1, 128, 2], n_sem=2, seed=903, second_round=False)
    s["zero_delta"] = dict(counts=[20, 70, 5, 6], n_sem=3, seed=904, zero_delta={0: 7, 1: 64, 2: 0})
    s["special"] = dict(counts=[90, 90, 90, 4], n_sem=3, seed=905)
    return s


def build_update_case(name):
    c = case_update(name, **update_case_specs()[name])
    if name == "special":
        # an opaque sample (200 > 88), a half-opaque one and sigma = 0 rows, with
        # the stop that follows from them
        _place(c, int(c.span[0, 0]), 30, 200.0)
        _place(c, int(c.span[1, 0]), 45, 30.0)
        c.sigmas[int(c.span[2, 0]):int(c.span[2, 0]) + 90:2] = 0
    return c


def update_args(c):
    return (c.n_alive, c.cap, c.rays_alive, c.rays_t, c.span, c.sigmas, c.sigma_scale, c.rgbs,
            c.local_sem, c.deltas, c.weights_sum, c.depth, c.image, c.semantics)


def steps_args(c):
    n_step, sig, rgb, ls, dl = as_steps(c)
    return (c.n_alive, n_step, c.rays_alive, c.rays_t, sig, rgb, ls, dl, c.weights_sum, c.depth,
            c.image, c.semantics)


def check_pinned(sw, what):
    """no stop and no mask decision within its bound of the threshold"""
    assert not sw.near_T.any(), f"{what}: T within its bound of 1e-4 at {np.argwhere(sw.near_T)[:4].tolist()}"
    assert not sw.near_w.any(), f"{what}: w within its bound of w_min at {np.argwhere(sw.near_w)[:4].tolist()}"


def check_stops(c, sw):
    """the placed stops are where they were asked for, by the margins asked for"""
    T = np.asarray(sw.T, F64)
    for s, k in getattr(c, "stops", {}).items():
        if s < sw.n:
            assert T[s, k - 1] >= 1e-2 and T[s, k] <= 1e-6, (c.name, s, k, T[s, k - 1], T[s, k])
            assert sw.used[s, k] and not sw.used[s, k + 1:].any()


# ---------------------------------------------------------------------------
# cases of the fused kernels
# ---------------------------------------------------------------------------
CLASS_COUNTS = (1, 15, 16, 17, 40, 61)
W_MINS = (0.0, 1e-4)
FUSED_KEYS = ("weights_sum", "depth", "image", "semantics", "rays_t")
MARCH_FWD_KEYS = ("weights_sum", "depth", "image", "semantics", "w_out", "t_out")
MARCH_BWD_KEYS = ("G", "d_h", "dW_color", "dW_sem")


def rays_per_wave(n_cap):
    """slots one wave of the fused kernels owns (composite.hip, march_shade_launch)"""
    return min(max(2, -(-n_cap // (256 * CMP_WAVES))), RPW_MAX)


def _pin_gates(c, rng, mode):
    """redraw the h row of every sample with a hidden pre-activation within its
    bound of zero (``shade_numpy.pin_case``'s rule) -> share redrawn"""
    nets = [(mode, split_nets(c.color_params, c.sem_params, c.C, mode))]
    dirs = c.rays_d[c.sample_ray]
    idx = np.arange(c.M)
    red = np.zeros(c.M, bool)
    for _ in range(100):
        if idx.size == 0:
            break
        bad = sn._gate_offenders(dirs[idx], c.h[idx, 1:], nets, c.C)
        idx = idx[bad]
        red[idx] = True
        c.h[idx, 1:] = rng.standard_normal((idx.size, 15)).astype(F32)
    else:
        raise AssertionError("gates not pinned after 100 rounds")
    return red


def case_fused(name, counts, C, w_min, mode, seed=0, stops=(), head_stop=(), cap=None, n_alive=None,
               sigma_scale=0.85, second_round=True, all_kept=(), none_kept=(), faint=(), tight_stop=(),
               color_params=None, sem_params=None):
    """``ucsa_march_segment_shade*``: slots in order with contiguous spans (an
    empty slot carries the offset of the next one, as the exclusive prefix sums
    of ``ucsa_march_segment_count`` do), a wave owns ``rays_per_wave(n_cap)``
    consecutive slots.  ``all_kept`` slots have alpha ~ 2 / count everywhere
    (every sample above 1e-4: the pending list drains in mid-ray), ``none_kept``
    slots sigma = 0 throughout, ``faint`` slots alpha = 6e-5 on every other
    sample (used, but below a w_min of 1e-4: weights_sum and the masked sums part).  Gates and the w_min mask are pinned at ``mode``."""
    rng = np.random.default_rng(seed + 17)
    c = case_update(name, counts, 0, seed, stops=stops, head_stop=head_stop, cap=cap,
                    sigma_scale=sigma_scale, second_round=second_round, tight_stop=tight_stop)
    c.C, c.w_min, c.mode = C, float(w_min), mode
    c.color_params, c.sem_params = color_params, sem_params
    if n_alive is not None:
        c.n_alive = n_alive
    N, M = c.N, c.M
    d = rng.standard_normal((N, 3))
    c.rays_d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    c.h = rng.standard_normal((M, 16)).astype(F32)
    c.semantics = (0.5 * rng.random((N, C))).astype(F32) if second_round else np.zeros((N, C), F32)
    cnt, off = c.span[:, 1].astype(np.int64), c.span[:, 0].astype(np.int64)
    c.sample_ray = np.repeat(c.rays_alive.astype(np.int64), cnt)
    for s in all_kept:
        k = int(cnt[s])
        al = (1.5 + rng.random(k)) / k
        c.sigmas[off[s]:off[s] + k] = (-np.log1p(-al) / (c.deltas[off[s]:off[s] + k, 0] * c.sigma_scale)).astype(F32)
    for s in none_kept:
        c.sigmas[off[s]:off[s] + cnt[s]] = 0
    for s in faint:
        _faint(c, off[s], cnt[s])
    red = _pin_gates(c, rng, mode)
    # the mask: redraw the sigma of a sample whose weight is within its bound of
    # w_min (never a placed one: those weights are far from 1e-4)
    for _ in range(100):
        sw = _fused_weights(c)
        bad = sw.near_w
        if not bad.any():
            break
        pi, _ = pad_spans(off[:c.n_alive], cnt[:c.n_alive])
        m = pi[bad]
        red[m] = True
        c.sigmas[m] = (c.sigmas[m] * (0.5 + rng.random(m.size))).astype(F32)
    else:
        raise AssertionError("mask not pinned after 100 rounds")
    c.h[:, 0] = np.log(np.maximum(c.sigmas, F32(1e-30)))
    c.redrawn = float(red.mean()) if M else 0.0
    if c.redrawn > REDRAW_CAP:
        raise RedrawCap(f"{name} at the {mode} margin: {c.redrawn:.1%} of the samples redrawn")
    return c


def _faint(c, off, cnt):
    m = np.arange(off, off + cnt, 2)
    c.sigmas[m] = (-math.log1p(-6e-5) / (c.deltas[m, 0] * c.sigma_scale)).astype(F32)


def _fused_weights(c):
    cnt, off = c.span[:c.n_alive, 1].astype(np.int64), c.span[:c.n_alive, 0].astype(np.int64)
    pi, valid = pad_spans(off, cnt)
    ra = c.rays_alive[:c.n_alive].astype(np.int64)
    return span_weights(_gather(c.sigmas, pi, valid, F64), _gather(c.deltas, pi, valid, F64),
                        t0=c.rays_t[:c.n_alive].astype(F64), sigma_scale=c.sigma_scale, stop=True,
                        w_min=c.w_min, valid=valid, ws0=c.weights_sum[ra].astype(F64))


def fused_case_specs():
    """name -> builder arguments.  With rays_per_wave = 2 (n_cap <= 6144) slots
    (2 i, 2 i + 1) share a wave."""
    s = {}
    s["single"] = dict(counts=[9])                   # n_cap = 1, 2, 3: one wave, its last slot
    s["two"] = dict(counts=[5, 7])                   # not alive from 2 on
    s["three"] = dict(counts=[5, 7, 3])
    # waves: (empty, 9) (9, empty) (empty, empty) (64, 64: a head at lane 0 of the
    # second chunk) (100, 30: cut by one boundary) (200, 10: by two, drains in
    # mid-ray) (sigma = 0: nothing kept) (150 all kept) + the slot not alive
    # (140 with every other sample faint) + the slot not alive
    s["layouts"] = dict(counts=[0, 9, 9, 0, 0, 0, 64, 64, 100, 30, 200, 10, 20, 20, 150, 6, 140, 3, 4],
                        all_kept=(10, 14), none_kept=(12, 13), stops={8: 70}, faint=(16,))
    # a stop-bearing slot is the first of its wave: its head sits at lane 0
    s["stops"] = dict(counts=[130, 4, 130, 4, 130, 4, 130, 4, 130, 4, 130, 2, 3],
                      stops={0: 62, 2: 63, 4: 64, 6: 128, 8: 129}, head_stop=(10,), tight_stop=(11,))
    s["cap_above"] = dict(counts=[12, 12, 3, 12, 2], cap=13)
    s["cap_equal"] = dict(counts=[12, 12, 3, 12, 2], cap=12, stops={1: 11})
    s["first_round"] = dict(counts=[64, 1, 128, 2, 1], second_round=False)
    s["alive_short"] = dict(counts=[8, 0, 70, 9, 5, 5, 5, 5], n_alive=3)
    return s


def build_fused_case(name, color_params, sem_params, mode, C=40, w_min=1e-4):
    a = dict(fused_case_specs()[name])
    for k in range(8):
        try:
            c = case_fused(name, C=C, w_min=w_min, mode=mode, seed=1000 + 10000 * k, color_params=color_params,
                           sem_params=sem_params, **a)
        except RedrawCap:
            continue
        assert c.redrawn <= REDRAW_CAP
        return c
    raise RedrawCap(f"{name}: no seed of 8 met the redraw cap at the {mode} margin")


def case_fused_wide(n_cap, color_params, sem_params, mode, C=40, w_min=1e-4, seed=0, max_count=2, fill=0.5):
    """many slots, a share ``fill`` of them with spans of 1 .. max_count samples,
    the others empty: n_cap = 6145 is the first rays_per_wave of 3 (empty slots
    in the MIDDLE of a wave's range), n_cap = 393,217 the first that would ask
    for 129 and is clamped to 128."""
    rng = np.random.default_rng(seed + n_cap)
    counts = rng.integers(1, max_count + 1, n_cap) * (rng.random(n_cap) < fill)
    counts[:6] = (0, 1, 0, max_count, 0, 1)
    return case_fused(f"wide{n_cap}", counts, C, w_min, mode, seed=seed + n_cap, n_alive=n_cap,
                      cap=max_count, color_params=color_params, sem_params=sem_params)


def fused_args(c):
    return (c.mode, c.n_alive, c.cap, c.rays_alive, c.rays_t, c.span, c.rays_d, c.sigmas, c.sigma_scale,
            c.h, c.deltas, c.color_params, c.sem_params, c.C, c.w_min, c.weights_sum, c.depth, c.image,
            c.semantics)


def case_march_train(name, counts, C, w_min, color_params, sem_params, seed=0, drop_last=False,
                     sigma_scale=0.85, all_kept=(), faint=()):
    """``ucsa_march_train_*``: rows of rays [N, 3] in point order (as
    ``ucsa_march_rays_train`` writes them) with permuted ray ids; the last span
    ends at M - 1, or at M with ``drop_last``.  Gates pinned at fp32; the
    forward's w_min mask pinned like the fused cases."""
    rng = np.random.default_rng(seed + 29)
    counts = np.asarray(counts, np.int64)
    N = len(counts)
    ray, sigma, deltas = _samples(rng, counts)
    total = int(counts.sum())
    M = total if drop_last else total + 1
    pad = M - total
    c = NS(name=name, N=N, M=M, C=C, w_min=float(w_min), sigma_scale=float(sigma_scale), mode=FP32,
           color_params=color_params, sem_params=sem_params)
    c.sigmas = np.concatenate([sigma / F32(sigma_scale), np.ones(pad, F32)]).astype(F32)
    c.deltas = np.concatenate([deltas, np.full((pad, 2), 0.01, F32)])
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for s in all_kept:
        k = int(counts[s])
        al = (1.5 + rng.random(k)) / k
        c.sigmas[off[s]:off[s] + k] = (-np.log1p(-al) / (c.deltas[off[s]:off[s] + k, 0] * c.sigma_scale)).astype(F32)
    for s in faint:
        _faint(c, off[s], counts[s])
    ids = rng.permutation(N)
    c.rays = np.stack([ids, off, counts], 1).astype(np.int32)
    c.nears = (0.2 + rng.random(N)).astype(F32)
    c.norms = (1.0 + 0.3 * rng.random(N)).astype(F32)
    d = rng.standard_normal((N, 3))
    c.rays_d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    c.h = rng.standard_normal((M, 16)).astype(F32)
    c.sample_ray = np.concatenate([np.repeat(ids, counts), np.zeros(pad, np.int64)])
    c.d_image = rng.standard_normal((N, 3)).astype(F32)
    c.d_depth = rng.standard_normal(N).astype(F32)
    c.d_sem = rng.standard_normal((N, C)).astype(F32)
    red = _pin_gates(c, rng, FP32)
    for _ in range(100):
        fw = march_train_weights(c)
        bad = fw.near_w
        if not bad.any():
            break
        pi, _ = pad_spans(off, np.where((off + counts >= M) | (counts > MAX_SPAN), 0, counts))
        m = pi[bad]
        red[m] = True
        c.sigmas[m] = (c.sigmas[m] * (0.5 + rng.random(m.size))).astype(F32)
    else:
        raise AssertionError("mask not pinned after 100 rounds")
    c.h[:, 0] = np.log(np.maximum(c.sigmas, F32(1e-30)))
    c.redrawn = float(red.mean())
    if c.redrawn > REDRAW_CAP:
        raise RedrawCap(f"{name}: {c.redrawn:.1%} of the samples redrawn")
    return c


def march_train_weights(c):
    idx, off, cnt = _train_rows(c.rays, c.M, (), limit=MAX_SPAN)
    pi, valid = pad_spans(off, cnt)
    return span_weights(_gather(c.sigmas, pi, valid, F64), _gather(c.deltas, pi, valid, F64),
                        t0=c.nears[idx].astype(F64), sigma_scale=c.sigma_scale, w_min=c.w_min, valid=valid)


def march_train_specs():
    s = {}
    s["small"] = dict(counts=[5, 0, 70, 9, 0, 130, 3, 90], faint=(7,))
    s["span1024"] = dict(counts=[3, 1024, 0, 66], all_kept=(1,))
    s["dropped_last"] = dict(counts=[7, 64, 0, 20], drop_last=True)
    s["span1025"] = dict(counts=[6, 1025, 65, 1024, 4])
    return s


def build_march_train_case(name, color_params, sem_params, C=40, w_min=1e-4):
    a = dict(march_train_specs()[name])
    for k in range(8):
        try:
            return case_march_train(name, C=C, w_min=w_min, color_params=color_params, sem_params=sem_params,
                                    seed=2000 + 10000 * k, **a)
        except RedrawCap:
            continue
    raise RedrawCap(f"{name}: no seed of 8 met the redraw cap")


def march_fwd_args(c):
    return (c.rays, c.M, c.nears, c.rays_d, c.sigmas, c.sigma_scale, c.h, c.deltas, c.color_params,
            c.sem_params, c.C, c.w_min)


def march_bwd_args(c, w_all, t_all):
    return (c.rays, c.M, c.rays_d, c.norms, c.sigmas, c.sigma_scale, c.h, c.deltas, w_all, t_all,
            c.color_params, c.sem_params, c.C, c.w_min, c.d_image, c.d_depth, c.d_sem)
