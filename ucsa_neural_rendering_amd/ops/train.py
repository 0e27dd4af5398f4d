"""Around the training step: Adam, the losses and post-processing, the
segmentation tail, fused BatchNorm, the confusion matrix and augmentation."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, lib
from ._args import _f32, _ptr, _scratch, _stream


def adam_step(p, g, m, v, step: int, lr: float, beta1: float, beta2: float,
              eps: float, weight_decay: float, inv_grad_scale: float = 1.0):
    for x in (p, g, m, v):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    check(lib().ucsa_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(),
                               int(step), float(lr), float(beta1), float(beta2),
                               float(eps), float(weight_decay),
                               float(inv_grad_scale), _stream()),
          "ucsa_adam_step")


def adam_step_scaled(p, g, m, v, step: int, lr: float, beta1: float,
                     beta2: float, eps: float, weight_decay: float,
                     grad_scale: torch.Tensor, found_inf: torch.Tensor,
                     skipped: torch.Tensor):
    """Adam step under GradScaler with the scale / found-inf flag on the
    device (no read-back); `skipped` int32[1] counts the skipped steps."""
    for x in (p, g, m, v):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    assert grad_scale.dtype == torch.float32 and found_inf.dtype == torch.float32
    assert skipped.dtype == torch.int32
    check(lib().ucsa_adam_step_scaled(
        _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), int(step), float(lr),
        float(beta1), float(beta2), float(eps), float(weight_decay),
        _ptr(grad_scale), _ptr(found_inf), _ptr(skipped), _stream()),
        "ucsa_adam_step_scaled")


def adam_count_skipped(found_inf: torch.Tensor, skipped: torch.Tensor):
    check(lib().ucsa_adam_count_skipped(_ptr(found_inf), _ptr(skipped),
                                        _stream()), "ucsa_adam_count_skipped")


# ===================== losses / post-processing / metric ====================
def nerf_loss(rgb, sem, depth, gt_rgb, labels, gt_depth, uom: float,
              w_sem: float = 0.04, w_depth: float = 0.1,
              grad_scale: float = 1.0, want_grad: bool = True):
    """-> stats[8] (device), (d_rgb, d_sem, d_depth) | None."""
    rgb = _f32(rgb, "rgb").view(-1, 3)
    N = rgb.shape[0]
    sem = _f32(sem, "sem").view(N, -1)
    Cn = sem.shape[1]
    depth = _f32(depth, "depth").view(N)
    gt_rgb = _f32(gt_rgb, "gt_rgb").view(N, 3)
    gt_depth = _f32(gt_depth, "gt_depth").view(N)
    labels = labels.reshape(N).to(torch.int64).contiguous()
    dev = rgb.device
    stats = torch.empty(8, device=dev)
    partial = torch.empty(int(lib().ucsa_loss_partial_floats(N)), device=dev)
    grads = None
    if want_grad:
        grads = (torch.empty_like(rgb), torch.empty_like(sem),
                 torch.empty_like(depth))
    check(lib().ucsa_nerf_loss(
        _ptr(rgb), _ptr(sem), _ptr(depth), _ptr(gt_rgb), _ptr(labels),
        _ptr(gt_depth), N, Cn, float(uom), float(w_sem), float(w_depth),
        float(grad_scale), _ptr(stats),
        _ptr(grads[0]) if grads else None, _ptr(grads[1]) if grads else None,
        _ptr(grads[2]) if grads else None, _ptr(partial), _stream()),
        "ucsa_nerf_loss")
    return stats, grads


def nerf_loss_apply(grads, g_total, g_color, g_sem, g_depth, w_sem: float,
                    w_depth: float):
    """``grads`` = (d_rgb [N,3], d_sem [N,C], d_depth [N]) of ``nerf_loss``
    times the loss node's cotangents (0-d / 1-element device tensors or None),
    one launch (ucsa_nerf_loss_apply) into FRESH tensors: ``grads`` are the
    tensors the autograd node saved and a second backward through a retained
    graph must find them unscaled (the in-place form scaled them
    twice, unseen by autograd's version counter)."""
    d_rgb, d_sem, d_depth = grads
    N, Cn = d_sem.shape
    out = torch.empty(N * (4 + Cn), dtype=torch.float32, device=d_rgb.device)
    o_rgb = out[:N * 3].view(N, 3)
    o_sem = out[N * 3:N * (3 + Cn)].view(N, Cn)
    o_depth = out[N * (3 + Cn):]

    def sc(t):
        if t is None:
            return None
        t = t.detach().reshape(-1)
        if not t.is_cuda or t.dtype != torch.float32 or t.numel() != 1:
            t = t.to(d_rgb.device, torch.float32).reshape(1)
        return t.contiguous()

    gt, gc, gs, gd = sc(g_total), sc(g_color), sc(g_sem), sc(g_depth)
    check(lib().ucsa_nerf_loss_apply(_ptr(d_rgb), _ptr(d_sem), _ptr(d_depth),
                                     _ptr(o_rgb), _ptr(o_sem), _ptr(o_depth), N, Cn,
                                     _ptr(gt), _ptr(gc), _ptr(gs), _ptr(gd),
                                     float(w_sem), float(w_depth), _stream()),
          "ucsa_nerf_loss_apply")
    return o_rgb, o_sem, o_depth


def semantic_postproc(sem, want_normalised: bool = True):
    """[..., C] -> (normalised [..., C] | None, argmax [...] int64)."""
    shape = sem.shape
    s = _f32(sem, "sem").view(-1, shape[-1])
    N, Cn = s.shape
    norm = torch.empty_like(s) if want_normalised else None
    arg = torch.empty(N, dtype=torch.int64, device=s.device)
    check(lib().ucsa_semantic_postproc(_ptr(s), N, Cn, _ptr(norm), _ptr(arg),
                                       _stream()), "ucsa_semantic_postproc")
    return (None if norm is None else norm.view(shape)), arg.view(shape[:-1])


def seg_tail(logits, labels=None, grad_scale: float = 1.0,
             want_prob: bool = True, want_grad: bool = False):
    """logits [B,C,H,W] -> dict(prob, argmax, loss, d_logits)."""
    x = _f32(logits, "logits")
    B, Cn, H, W = x.shape
    P = H * W
    dev = x.device
    prob = torch.empty_like(x) if want_prob else None
    arg = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    loss = d_logits = partial = None
    if labels is not None:
        labels = labels.reshape(B, P).to(torch.int64).contiguous()
        loss = torch.empty(1, device=dev)
        partial = torch.empty(int(lib().ucsa_loss_partial_floats(B * P)),
                              device=dev)
        if want_grad:
            d_logits = torch.empty_like(x)
    check(lib().ucsa_seg_tail(_ptr(x), _ptr(labels), B, Cn, P,
                              float(grad_scale), _ptr(prob), _ptr(arg),
                              _ptr(loss), _ptr(d_logits), _ptr(partial),
                              _stream()), "ucsa_seg_tail")
    return dict(prob=prob, argmax=arg, loss=loss, d_logits=d_logits)


# ---------------------------------------------------------------------------
# fused BatchNorm2d (+ residual) (+ ReLU) on channels-last activations
# ---------------------------------------------------------------------------
def _nhwc_rows(t: torch.Tensor, name: str):
    """[N,C,H,W] channels_last tensor (fp32 / bf16) -> (M, C, dtype code)."""
    if not t.is_cuda:
        raise _lib.UcsaError(f"{name} must live on the GPU: no CPU fallback")
    if t.dim() != 4 or not t.is_contiguous(memory_format=torch.channels_last):
        raise _lib.UcsaError(f"{name} must be a channels_last [N,C,H,W] tensor")
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.UcsaError(f"{name}: fp32 or bf16, got {t.dtype}")
    N, Cc, H, W = t.shape
    return N * H * W, Cc, 0 if t.dtype == torch.float32 else 1


BN_MAX_CHANNELS = 4096   # csrc/batchnorm.hip: per-workgroup column tables


def _bn_vec(t, name: str, Cc: int, device):
    """A per-channel operand of the BatchNorm kernels, which read ``float*`` of
    length C: fp32, contiguous, on x's device -- or None.  (A ``model.half()``
    / ``.bfloat16()`` module has 2-byte parameters: handing those over would be
    an out-of-bounds read and silently wrong statistics.)"""
    if t is None:
        return None
    if (t.dtype != torch.float32 or t.device != device or not t.is_contiguous()
            or t.numel() != Cc):
        raise _lib.UcsaError(
            f"bn_act: {name} must be a contiguous fp32 [{Cc}] tensor on {device}, got "
            f"{t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def bn_vec_ok(t, Cc: int, device) -> bool:
    return t is None or (t.dtype == torch.float32 and t.device == device
                         and t.is_contiguous() and t.numel() == Cc)


def bn_act_fwd(x, residual, weight, bias, running_mean, running_var,
               momentum: float, eps: float, relu: bool, training: bool):
    """-> (y, save_mean, save_invstd); save_* are None in eval mode."""
    M, Cc, dt = _nhwc_rows(x, "x")
    if Cc > BN_MAX_CHANNELS:
        raise _lib.UcsaError(f"bn_act: C = {Cc} > {BN_MAX_CHANNELS}")
    for name, v in (("weight", weight), ("bias", bias), ("running_mean", running_mean),
                    ("running_var", running_var)):
        _bn_vec(v, name, Cc, x.device)
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or
                                 not residual.is_contiguous(memory_format=torch.channels_last)):
        raise _lib.UcsaError("residual must match x (shape, dtype, channels_last)")
    y = torch.empty_like(x)   # preserves channels_last
    save_mean = save_invstd = None
    if training:
        save_mean = torch.empty(Cc, device=x.device)
        save_invstd = torch.empty(Cc, device=x.device)
    ws = _scratch(int(lib().ucsa_bn_workspace_bytes(M, Cc)), x.device)
    check(lib().ucsa_bn_act_fwd(
        _ptr(x), _ptr(residual), _ptr(weight), _ptr(bias), _ptr(running_mean),
        _ptr(running_var), float(momentum), float(eps), M, Cc, int(relu),
        int(training), dt, _ptr(y), _ptr(save_mean), _ptr(save_invstd), _ptr(ws),
        _stream()), "ucsa_bn_act_fwd")
    return y, save_mean, save_invstd


def bn_act_bwd(dy, x, y, weight, save_mean, save_invstd, relu: bool,
               want_dres: bool, want_dwb: bool):
    """-> (dx, dresidual | None, dweight | None, dbias | None)."""
    M, Cc, dt = _nhwc_rows(x, "x")
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise _lib.UcsaError("dy must match x")
    for name, v in (("weight", weight), ("save_mean", save_mean), ("save_invstd", save_invstd)):
        _bn_vec(v, name, Cc, x.device)
    if relu and (y is None or y.dtype != x.dtype or y.shape != x.shape or
                 not y.is_contiguous(memory_format=torch.channels_last)):
        raise _lib.UcsaError("bn_act_bwd: y must match x (relu mask)")
    dy = dy.contiguous(memory_format=torch.channels_last)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    dw = torch.empty(Cc, device=x.device) if want_dwb else None
    db = torch.empty(Cc, device=x.device) if want_dwb else None
    ws = _scratch(int(lib().ucsa_bn_workspace_bytes(M, Cc)), x.device)
    check(lib().ucsa_bn_act_bwd(
        _ptr(dy), _ptr(x), _ptr(y) if relu else None, _ptr(weight), _ptr(save_mean),
        _ptr(save_invstd), M, Cc, int(relu), dt, _ptr(dx), _ptr(dres), _ptr(dw),
        _ptr(db), _ptr(ws), _stream()), "ucsa_bn_act_bwd")
    return dx, dres, dw, db


def confusion_matrix(preds, truths, n_classes: int, cm=None):
    p = preds.reshape(-1).to(torch.int64).contiguous()
    t = truths.reshape(-1).to(torch.int64).contiguous()
    if not p.is_cuda:
        raise _lib.UcsaError("confusion_matrix needs GPU tensors")
    if cm is None:
        cm = torch.zeros(n_classes, n_classes, dtype=torch.int64,
                         device=p.device)
    check(lib().ucsa_confusion_matrix(_ptr(p), _ptr(t), p.numel(), n_classes,
                                      _ptr(cm), _stream()),
          "ucsa_confusion_matrix")
    return cm


def augment(img, label, params, out_size=None):
    """Rendered-image augmentation (ucsa_augment).  img [B,3,H,W] fp32 in
    [0,1], label [B,H,W] int64 or None, params: list of B dicts with keys
    order (4 ints), brightness, contrast, saturation, hue, angle_deg, flip,
    crop_i, crop_j.  -> out_img [B,3,oh,ow], out_label [B,oh,ow] | None."""
    img = _f32(img, "img")
    B, _, H, W = img.shape
    oh, ow = (H, W) if out_size is None else out_size
    if label is not None:
        if not (label.is_cuda and label.dtype == torch.int64):
            raise _lib.UcsaError("label must be an int64 tensor on the GPU")
        label = label.contiguous()
    if len(params) != B:
        raise _lib.UcsaError(f"params must have one entry per image: {len(params)} for B = {B}")
    if B == 0:      # an empty tensor has no data pointer to hand over
        return (img.new_empty(0, 3, oh, ow),
                None if label is None else label.new_empty(0, oh, ow))
    arr = (_lib.AugParams * B)()
    for k, q in enumerate(params):
        arr[k].order[:] = [int(v) for v in q["order"]]
        arr[k].brightness = float(q["brightness"])
        arr[k].contrast = float(q["contrast"])
        arr[k].saturation = float(q["saturation"])
        arr[k].hue = float(q["hue"])
        arr[k].angle_deg = float(q["angle_deg"])
        arr[k].flip = int(bool(q["flip"]))
        arr[k].crop_i = int(q.get("crop_i", 0))
        arr[k].crop_j = int(q.get("crop_j", 0))
    out = torch.empty(B, 3, oh, ow, device=img.device)
    out_l = (torch.empty(B, oh, ow, dtype=torch.int64, device=img.device)
             if label is not None else None)
    ws = _scratch(int(lib().ucsa_augment_workspace_bytes(B, H, W)), img.device)
    check(lib().ucsa_augment(_ptr(img), _ptr(label), B, H, W, arr, oh, ow,
                             _ptr(out), _ptr(out_l), _ptr(ws), _stream()),
          "ucsa_augment")
    return out, out_l
