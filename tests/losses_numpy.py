"""numpy float64 restatement of the loss / post-processing / metric / Adam
contracts of include/ucsa_hip.h (``ucsa_nerf_loss``, ``ucsa_nerf_loss_apply``,
``ucsa_semantic_postproc``, ``ucsa_seg_tail``, ``ucsa_confusion_matrix``,
``ucsa_adam_step`` and its GradScaler form), written from the formulas of
``oracle/losses.py`` and the header comments: closed-form values and gradients,
no autograd, no GPU, no HIP library (test infrastructure).  It knows nothing of
blocks, waves or grid strides.  ``tests/test_losses_reference_cpu.py`` holds it
against the oracle and the torch modules in float64.

Where the kernels deliberately differ from torch, the documented behaviour is
encoded here: a label outside ``[0, C)`` is IGNORED (torch's nll_loss raises on
a label >= C), like -1.

The second half builds the inputs both test files share.  Probabilities are
multiples of 1/1024 and logits multiples of 1/8: sums of a row are exact in
fp32, ties are exact and non-ties are far apart, so every argmax comparison is
exact and no row has to be excluded."""
import numpy as np

F64 = np.float64
LOG_EPS = 1e-15          # oracle/losses.py: log(sem + 1e-15)


def _f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, F64)


def _i64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.int64)


# ---------------------------------------------------------------------------
# NeRF losses
# ---------------------------------------------------------------------------
def nerf_loss_ref(rgb, sem, depth, gt_rgb, labels, gt_depth, uom, w_sem, w_depth):
    """-> (stats [8], (d_rgb [N,3], d_sem [N,C], d_depth [N])), float64.

    stats = {loss_color, loss_semantics (NaN = the reference's None),
    loss_depth (NaN without a pixel with depth), n_invalid_sem, n_valid_depth,
    total, loss_semantics with None as 0, 0}; the gradients are those of
    ``total = color + w_sem * sem + w_depth * depth`` where a skipped semantic
    term and an empty depth term contribute no gradient."""
    rgb, gt_rgb = _f64(rgb).reshape(-1, 3), _f64(gt_rgb).reshape(-1, 3)
    N = rgb.shape[0]
    sem = _f64(sem).reshape(N, -1)
    C = sem.shape[1]
    depth, gt_depth = _f64(depth).reshape(N), _f64(gt_depth).reshape(N)
    labels = _i64(labels).reshape(N)
    uom, w_sem, w_depth = float(uom), float(w_sem), float(w_depth)

    e = rgb - gt_rgb
    lc = np.mean(e * e)
    d_rgb = 2.0 * e / (3.0 * N)

    S = sem.sum(axis=1)
    invalid = S == 0
    n_invalid = int(invalid.sum())
    sem_ok = n_invalid < N
    use = ~invalid & (labels >= 0) & (labels < C)    # rows with a loss term
    d_sem = np.zeros_like(sem)
    ls = np.nan
    if sem_ok:
        r = np.nonzero(use)[0]
        lab = labels[r]
        pl = sem[r, lab] / S[r]
        ls = float(np.sum(-np.log(pl + LOG_EPS)) / N)     # ignored rows count as 0
        # d/ds_k of -log(s_l / S + eps) = -(delta_kl - p_l) / ((p_l + eps) S)
        coef = -w_sem / (N * (pl + LOG_EPS) * S[r])
        rows = -coef[:, None] * pl[:, None] * np.ones((1, C))
        rows[np.arange(r.size), lab] = coef * (1.0 - pl)
        d_sem[r] = rows

    valid = gt_depth != 0
    n_valid = int(valid.sum())
    d_depth = np.zeros(N)
    ld = np.nan
    if n_valid:
        ed = depth[valid] / uom - gt_depth[valid]
        ld = float(np.mean(np.abs(ed)))
        d_depth[valid] = w_depth * np.sign(ed) / (uom * n_valid)

    total = lc + (ls * w_sem if sem_ok else 0.0) + ld * w_depth
    stats = np.array([lc, ls, ld, n_invalid, n_valid, total, ls if sem_ok else 0.0, 0.0], F64)
    return stats, (d_rgb, d_sem, d_depth)


def nerf_loss_apply_ref(grads, g_total, g_color, g_sem, g_depth, w_sem, w_depth):
    """The stored gradients of the weighted total times the cotangents of the
    total and of the single terms (None = 0); a term's own gradient is the stored
    one over its weight."""
    d_rgb, d_sem, d_depth = (_f64(g) for g in grads)
    s = lambda t: 0.0 if t is None else float(_f64(t).reshape(-1)[0])
    gt = s(g_total)
    return (d_rgb * (gt + s(g_color)), d_sem * (gt + s(g_sem) / float(w_sem)),
            d_depth * (gt + s(g_depth) / float(w_depth)))


def semantic_postproc_ref(sem):
    """[..., C] -> (normalised rows, first-maximum argmax); a row summing to 0
    becomes uniform."""
    sem = _f64(sem)
    S = sem.sum(axis=-1, keepdims=True)
    invalid = S == 0
    C = sem.shape[-1]
    norm = np.where(invalid, 1.0 / C, sem / np.where(invalid, 1.0, S))
    return norm, np.argmax(norm, axis=-1).astype(np.int64)


# ---------------------------------------------------------------------------
# segmentation tail
# ---------------------------------------------------------------------------
def seg_tail_ref(logits, labels=None, grad_scale=1.0):
    """logits [B,C,H,W], labels [B,H,W] -> dict(prob, argmax, loss, d_logits).
    loss = mean over ALL B*H*W pixels of CrossEntropy(softmax(logits), label),
    i.e. logsumexp(prob) - prob[label], an ignored pixel (label < 0 or >= C)
    counting as 0; d_logits = grad_scale * dloss/dlogits."""
    x = _f64(logits)
    B, C, H, W = x.shape
    z = x - x.max(axis=1, keepdims=True)
    ez = np.exp(z)
    p = ez / ez.sum(axis=1, keepdims=True)
    out = dict(prob=p, argmax=np.argmax(x, axis=1).astype(np.int64), loss=None, d_logits=None)
    if labels is None:
        return out
    lab = _i64(labels).reshape(B, H, W)
    ok = (lab >= 0) & (lab < C)
    total = B * H * W
    m2 = p.max(axis=1, keepdims=True)
    e2 = np.exp(p - m2)
    s2 = e2.sum(axis=1, keepdims=True)
    q = e2 / s2                                     # the second softmax
    lse = (m2 + np.log(s2))[:, 0]
    onehot = np.zeros_like(p)
    b, h, w = np.nonzero(ok)
    onehot[b, lab[b, h, w], h, w] = 1.0
    out["loss"] = float(np.sum(np.where(ok, lse - (p * onehot).sum(axis=1), 0.0)) / total)
    g = np.where(ok[:, None], q - onehot, 0.0) / total        # dloss/dprob
    out["d_logits"] = float(grad_scale) * p * (g - (p * g).sum(axis=1, keepdims=True))
    return out


# ---------------------------------------------------------------------------
# confusion matrix
# ---------------------------------------------------------------------------
def confusion_ref(preds, truths, C, cm0=None):
    """rows = truth; a pair with either value outside [0, C) is dropped."""
    p, t = _i64(preds).reshape(-1), _i64(truths).reshape(-1)
    cm = np.zeros((C, C), np.int64) if cm0 is None else _i64(cm0).copy()
    ok = (p >= 0) & (p < C) & (t >= 0) & (t < C)
    np.add.at(cm, (t[ok], p[ok]), 1)
    return cm


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
def adam_ref(p, g, m, v, step, lr, b1, b2, eps, wd, inv_scale=1.0):
    """One torch.optim.Adam update (non-AMSGrad, L2 decay in the gradient) of
    gradients ``g * inv_scale``; ``step`` is 1-based.  -> new (p, m, v)."""
    p, g, m, v = _f64(p), _f64(g) * float(inv_scale), _f64(m), _f64(v)
    if wd != 0.0:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step
    bc2 = 1.0 - b2 ** step
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adam_scaled_ref(p, grads, m, v, found_inf, grad_scale, lr, b1, b2, eps, wd):
    """The GradScaler form over ``len(grads)`` optimizer steps: step k (1-based)
    with ``found_inf[k-1] != 0`` leaves p, m and v untouched and does not count,
    the others divide the gradient by ``grad_scale[k-1]`` and use
    ``k - skipped`` in the bias corrections.  -> (per-step list of (p, m, v),
    skipped)."""
    p, m, v = _f64(p), _f64(m), _f64(v)
    skipped, hist = 0, []
    for k, g in enumerate(grads, 1):
        if found_inf[k - 1] != 0:
            skipped += 1
        else:
            p, m, v = adam_ref(p, g, m, v, k - skipped, lr, b1, b2, eps, wd,
                               1.0 / float(grad_scale[k - 1]))
        hist.append((p, m, v))
    return hist, skipped


# ===========================================================================
# shared inputs (float32 / int64 numpy, seeded)
# ===========================================================================
NERF_UOM = 0.7
# every N and every C of the issue's lists appears at least once
NERF_SHAPES = [(1, 1), (1, 40), (63, 3), (64, 64), (65, 1), (255, 40), (256, 3),
               (257, 40), (257, 64), (1029, 1), (1029, 40), (1029, 64)]
NERF_SPECIAL = [(257, 40, "no_depth"), (65, 3, "all_invalid")]


def prob_grid(rng, shape, zero_share=0.3):
    """Composited probabilities on the 1/1024 grid, a share of exact zeros."""
    k = rng.integers(0, 1025, size=shape)
    k[rng.random(shape) < zero_share] = 0
    return (k / 1024.0).astype(np.float32)


def nerf_case(N, C, kind="plain", seed=0):
    """dict of rgb, sem, depth, gt_rgb, labels, gt_depth (leading batch dim 1)
    and the row sets a test wants to look at.  As far as N and C leave room:
    all-zero rows (every 11th), labels -1, C and C+5, a valid row whose labelled
    class has probability exactly 0 (needs C > 1), gt_depth == 0 on a stride of
    9.  kind "no_depth": every gt_depth 0; "all_invalid": every row zero."""
    rng = np.random.default_rng(1000 * N + C + 7919 * seed)
    rgb = rng.random((N, 3), dtype=np.float32)
    gt_rgb = rng.random((N, 3), dtype=np.float32)
    sem = prob_grid(rng, (N, C))
    labels = rng.integers(-1, C, size=N).astype(np.int64)
    depth = rng.random(N, dtype=np.float32) * 3
    gt_depth = rng.random(N, dtype=np.float32) * 3 + np.float32(0.01)
    if N > 1:
        sem[1::11] = 0
        gt_depth[::9] = 0
    else:
        sem[0, 0] = np.float32(0.375)             # the only row is a valid one
    for i, l in ((2, -1), (3, C), (4, C + 5)):
        if N > i:
            labels[i] = l
    zero_prob_row = None
    if N > 5 and C > 1:
        zero_prob_row = 5
        sem[5] = (rng.integers(1, 1025, size=C) / 1024.0).astype(np.float32)
        labels[5] = C - 1
        sem[5, C - 1] = 0
    if kind == "no_depth":
        gt_depth[:] = 0
    elif kind == "all_invalid":
        sem[:] = 0
    else:
        assert kind == "plain"
    # the sign of depth / uom - gt_depth must not hang on fp32 rounding
    e = depth.astype(F64) / NERF_UOM - gt_depth
    assert np.all(np.abs(e[gt_depth != 0]) > 1e-5)
    S = sem.astype(F64).sum(1)
    lab_ok = (labels >= 0) & (labels < C) & (S != 0)
    pl = np.where(lab_ok, sem[np.arange(N), np.clip(labels, 0, C - 1)], 1.0)
    return dict(rgb=rgb[None], sem=sem[None], depth=depth[None], gt_rgb=gt_rgb[None],
                labels=labels[None], gt_depth=gt_depth[None], uom=NERF_UOM,
                zero_prob_row=zero_prob_row,
                huge_rows=np.nonzero(lab_ok & (pl == 0))[0])


def oracle_labels(labels, C):
    """Labels for torch's nll_loss / CrossEntropyLoss, which raise on a label
    >= C where the kernels ignore it: out-of-range -> -1."""
    labels = np.asarray(labels)
    return np.where((labels < 0) | (labels >= C), -1, labels).astype(np.int64)


SEG_SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (2, 40, 17, 23), (3, 21, 9, 31), (1, 64, 16, 17)]
SEG_CASES = ([(s, sc, "random") for s in SEG_SHAPES for sc in (3, 80)] +
             [((2, 40, 17, 23), 3, "all_ignored"), ((2, 40, 17, 23), 0, "random"),
              ((2, 40, 17, 23), 3, "ties"), ((3, 21, 9, 31), 80, "ties")])


def seg_case(shape, scale, kind, seed=0):
    """logits on the 1/8 grid (scale 0: every logit equal), labels in [-1, C)
    with some >= C.  kind "ties": in every third pixel the top two classes tie
    exactly; "all_ignored": every label -1."""
    B, C, H, W = shape
    rng = np.random.default_rng(B * 1000003 + C * 1009 + H * 31 + W + scale * 7 + seed)
    if scale == 0:
        x = np.full(shape, 1.625, np.float32)
    else:
        x = (np.round(rng.standard_normal(shape) * scale * 8) / 8).astype(np.float32)
    labels = rng.integers(-1, C, size=(B, H, W)).astype(np.int64)
    flat = labels.reshape(-1)
    flat[::7] = C
    flat[3::13] = C + 5
    if flat.size > 1:
        flat[1] = -1
    if kind == "ties" and C > 1:
        xf = x.transpose(0, 2, 3, 1).reshape(-1, C)        # a copy
        top = xf.argmax(1)
        other = (top + 1 + rng.integers(0, C - 1, size=top.size)) % C
        rows = np.arange(0, top.size, 3)
        xf[rows, other[rows]] = xf[rows, top[rows]]
        x = np.ascontiguousarray(xf.reshape(B, H, W, C).transpose(0, 3, 1, 2))
    elif kind == "all_ignored":
        labels[:] = -1
    return x, labels


def postproc_case(N, C, seed=0):
    """Rows on the 1/1024 grid: all-zero rows, exact ties of the maximum at
    several positions, rows with a single non-zero entry."""
    rng = np.random.default_rng(77 * N + C + seed)
    s = prob_grid(rng, (N, C))
    for i in range(N):
        k = i % 8
        if k == 1:
            s[i] = 0
        elif k == 2:
            s[i] = 0
            s[i, rng.integers(0, C)] = np.float32(rng.integers(1, 1025) / 1024.0)
        elif k in (3, 4, 5) and C > 1:
            top = s[i].max() if s[i].max() > 0 else np.float32(0.5)
            idx = rng.choice(C, size=min(C, k - 1), replace=False)
            s[i, idx] = top                       # 2, 3 or 4 equal maxima
    return s


def confusion_case(n, C, seed=0):
    """Pairs mostly inside [0, C), and -1, C, 255, 2**40 and -2**40 on either
    side (2**40 is 0 modulo 2**32: a 32-bit comparison would count it)."""
    rng = np.random.default_rng(13 * n + C + seed)
    p = rng.integers(0, C, size=n).astype(np.int64)
    t = rng.integers(0, C, size=n).astype(np.int64)
    bad = np.array([-1, C, 255, 2 ** 40, -2 ** 40], np.int64)
    if n == 1:
        return p, t
    k = max(2, n // 50)
    ip, it = rng.choice(n, k, replace=False), rng.choice(n, k, replace=False)
    p[ip] = bad[np.arange(k) % 5]
    t[it] = bad[(np.arange(k) + 2) % 5]
    return p, t


def adam_grads(rng, n):
    """fp32 gradients with magnitudes spread over [1e-12, 1e3], both signs, and
    exact zeros.  (Nothing in the range where g*g underflows fp32: what happens
    there is a property of fp32 Adam, not of a kernel.)"""
    mag = 10.0 ** rng.uniform(-12.0, 3.0, size=n)
    g = (mag * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    g[rng.random(n) < 0.05] = 0
    return g


# ===========================================================================
# the same formulas through the oracle / the torch modules at a chosen dtype:
# float64 to hold this file's closed forms against (test_losses_reference_cpu),
# float32 as the yardstick of what fp32 arithmetic costs (test_gpu_small_kernels)
# ===========================================================================
def torch_nerf(case, dtype, w_sem, w_depth):
    """oracle.losses.nerf_losses + autograd -> (stats[0..6] like the kernel's,
    NaN where the reference has None / an empty mean; gradients of the total,
    zeros where autograd has none)."""
    import torch
    from oracle import losses as ol
    C = case["sem"].shape[-1]
    t = lambda k: torch.from_numpy(case[k]).to(dtype)
    a = [t(k).requires_grad_() for k in ("rgb", "sem", "depth")]
    labels = torch.from_numpy(oracle_labels(case["labels"], C))
    lc, ls, ld = ol.nerf_losses(a[0], a[1], a[2], t("gt_rgb"), labels, t("gt_depth"),
                                case["uom"])
    total = lc
    if ls is not None:
        total = total + ls * w_sem
    total = total + ld * w_depth
    total.backward()
    S = a[1].detach().sum(-1)
    nan = float("nan")
    lc, ld, total = lc.detach(), ld.detach(), total.detach()
    ls = None if ls is None else ls.detach()
    stats = np.array([float(lc), nan if ls is None else float(ls), float(ld),
                      float((S == 0).sum()), float((t("gt_depth") != 0).sum()),
                      float(total), 0.0 if ls is None else float(ls)], F64)
    grads = tuple(np.zeros(x.shape[1:], F64) if x.grad is None else _f64(x.grad[0])
                  for x in a)
    return stats, grads


def torch_seg(x, labels, dtype, grad_scale=1.0):
    """F.softmax then CrossEntropyLoss(ignore_index=-1, reduction="none").mean()
    and autograd, as the reference configures them."""
    import torch
    import torch.nn.functional as F
    C = x.shape[1]
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    pred = F.softmax(xt, dim=1)
    lab = torch.from_numpy(oracle_labels(labels, C))
    loss = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")(pred, lab).mean()
    (loss * grad_scale).backward()
    return dict(prob=_f64(pred), argmax=torch.argmax(pred, dim=1).numpy(),
                loss=float(loss.detach()), d_logits=_f64(xt.grad))
