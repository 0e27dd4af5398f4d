"""Training backward: transposed packs, gradient reductions, the sigma-MLP,
hash-grid and composite backward passes and the fused training step."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from .. import _lib
from .._lib import Grid, check, fvec, lib
from ._args import _f32, _ptr, _raw_current_stream, _scratch_named, _stream
from .render import _mlp_pack


def mlp_pack_t(kind: int, params: torch.Tensor, n_classes: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _mlp_pack("ucsa_mlp_pack_t", kind, params, n_classes, out, "ucsa_mlp_pack_t_size")


def reduce_partials(partial: torch.Tensor, grad: torch.Tensor,
                    accumulate: bool):
    n_parts, n_params = partial.shape
    check(lib().ucsa_reduce_partials(_ptr(partial), n_parts, n_params,
                                     1 if accumulate else 0, _ptr(grad),
                                     _stream()), "ucsa_reduce_partials")


def reduce_partials_multi(pairs, accumulate: bool = False):
    """[(partial [parts, n], grad [n]), ...] (<= 4 pairs) in one launch."""
    k = len(pairs)
    P = (C.c_void_p * k)(*[p.data_ptr() for p, _ in pairs])
    G = (C.c_void_p * k)(*[g.data_ptr() for _, g in pairs])
    NP = (C.c_uint32 * k)(*[p.shape[0] for p, _ in pairs])
    NN = (C.c_uint32 * k)(*[p.shape[1] for p, _ in pairs])
    check(lib().ucsa_reduce_partials_multi(k, P, NP, NN, G,
                                           1 if accumulate else 0, _stream()),
          "ucsa_reduce_partials_multi")


def sigma_mlp_bwd(feat, d_h, packed_sigma, packed_sigma_t, x2: bool = False,
                  round_hidden: bool = False):
    """-> d_feat [L,M,2], dW partials [parts, 3072].  x2: the bf16x2 kernel
    (packed weights from mlp_pack_x3 / mlp_pack_t_x3); round_hidden: the fp32
    kernel with its recomputed hidden layer rounded to fp16 (tcnn numerics)."""
    L, M, _ = feat.shape
    d_feat = torch.empty_like(feat)
    parts = int(lib().ucsa_sigma_mlp_bwd_parts(M))
    partial = torch.empty(parts, 3072, device=feat.device)
    fn, nm = ((lib().ucsa_sigma_mlp_bwd_x2, "ucsa_sigma_mlp_bwd_x2") if x2 else
              (lib().ucsa_sigma_mlp_bwd_h16, "ucsa_sigma_mlp_bwd_h16") if round_hidden else
              (lib().ucsa_sigma_mlp_bwd, "ucsa_sigma_mlp_bwd"))
    check(fn(_ptr(feat), _ptr(d_h), _ptr(packed_sigma), _ptr(packed_sigma_t), M, L,
             _ptr(d_feat), _ptr(partial), _stream()), nm)
    return d_feat, partial


_bwd_ws = {}


def hashgrid_bwd_rays(grid: Grid, rays_o, rays_d, z, aabb, d_feat, grad_table,
                      binned: bool = True, rec_scale: float = 0.0,
                      packed: bool = False):
    """Adds the table gradient.  binned=True: two-pass LDS-binned algorithm
    (workspace cached per device); False: direct float atomics.
    rec_scale > 0 (binned only): 8-byte bin records, values as half2 x
    rec_scale (the f16 training mode).  packed (binned only): 8-byte records
    with 26-bit values (ucsa_hashgrid_bwd_rays_p64)."""
    N, T = z.shape
    if tuple(d_feat.shape) != (grid.n_levels, N * T, 2) or not d_feat.is_contiguous():
        raise _lib.UcsaError(
            f"d_feat must be a contiguous [{grid.n_levels}, {N * T}, 2] tensor "
            f"(levels, N*T samples of z {tuple(z.shape)}, 2), got {tuple(d_feat.shape)}")
    if tuple(rays_o.shape) != (N, 3) or tuple(rays_d.shape) != (N, 3):
        raise _lib.UcsaError("rays_o / rays_d must be [N, 3] with N = z.shape[0]")
    ws = None
    if binned:
        need = int(lib().ucsa_hashgrid_bwd_workspace_bytes(N, T, grid.n_levels))
        key = (z.device, _raw_current_stream())   # one bin buffer per stream
        ws = _bwd_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=z.device)
            _bwd_ws[key] = ws
    if rec_scale > 0.0 and ws is not None:
        check(lib().ucsa_hashgrid_bwd_rays_h16(
            C.byref(grid), _ptr(rays_o), _ptr(rays_d), _ptr(z), fvec(aabb), N, T,
            _ptr(d_feat), _ptr(grad_table), _ptr(ws), float(rec_scale), _stream()),
            "ucsa_hashgrid_bwd_rays_h16")
        return
    if packed and ws is not None:
        check(lib().ucsa_hashgrid_bwd_rays_p64(
            C.byref(grid), _ptr(rays_o), _ptr(rays_d), _ptr(z), fvec(aabb), N, T,
            _ptr(d_feat), _ptr(grad_table), _ptr(ws), _stream()),
            "ucsa_hashgrid_bwd_rays_p64")
        return
    check(lib().ucsa_hashgrid_bwd_rays(C.byref(grid), _ptr(rays_o),
                                       _ptr(rays_d), _ptr(z), fvec(aabb), N, T,
                                       _ptr(d_feat), _ptr(grad_table),
                                       _ptr(ws), _stream()),
          "ucsa_hashgrid_bwd_rays")


def hashgrid_bwd_rays_det(grid: Grid, rays_o, rays_d, z, aabb, d_feat, fix=None):
    """Deterministic accumulation of the table gradient of one density pass
    into the int64 fixed-point buffer ``fix`` (created zeroed when None;
    ucsa_hashgrid_bwd_rays_det).  Finish with ``hashgrid_bwd_det_finish``."""
    N, T = z.shape
    if tuple(d_feat.shape) != (grid.n_levels, N * T, 2) or not d_feat.is_contiguous():
        raise _lib.UcsaError("d_feat must be a contiguous [L, N*T, 2] tensor")
    if fix is None:
        n = int(lib().ucsa_hashgrid_bwd_det_workspace_bytes(C.byref(grid))) // 8
        fix = torch.zeros(n, dtype=torch.int64, device=z.device)
    check(lib().ucsa_hashgrid_bwd_rays_det(
        C.byref(grid), _ptr(rays_o), _ptr(rays_d), _ptr(z), fvec(aabb), N, T,
        _ptr(d_feat), _ptr(fix), _stream()), "ucsa_hashgrid_bwd_rays_det")
    return fix


def hashgrid_bwd_det_finish(grid: Grid, fix, grad_table):
    """grad_table += fix * 2^-44 (NaN everywhere after a non-finite contribution)."""
    check(lib().ucsa_hashgrid_bwd_det_finish(C.byref(grid), _ptr(fix), _ptr(grad_table),
                                             _stream()), "ucsa_hashgrid_bwd_det_finish")


def hashgrid_bwd_rays_merged(grid: Grid, rays_o, rays_d, z_c, z_f, src, aabb,
                             d_feat_c, d_feat_f, grad_table, packed: bool = False,
                             rec_scale: float = 0.0):
    """Both density passes in one call, every ray's samples walked in sorted
    depth order (``src`` [N, Tc+Tf] int32 of the forward composite): adds the
    table gradient (ucsa_hashgrid_bwd_rays_merged; packed: its _p64 form with
    8-byte records of 26-bit values)."""
    N, Tc = z_c.shape
    Tf = z_f.shape[1]
    L = grid.n_levels
    if (tuple(d_feat_c.shape) != (L, N * Tc, 2) or tuple(d_feat_f.shape) != (L, N * Tf, 2)
            or not d_feat_c.is_contiguous() or not d_feat_f.is_contiguous()):
        raise _lib.UcsaError("d_feat_c / d_feat_f must be contiguous [L, N*T, 2] tensors")
    if tuple(src.shape) != (N, Tc + Tf) or src.dtype != torch.int32 or not src.is_contiguous():
        raise _lib.UcsaError(f"src must be a contiguous int32 [{N}, {Tc + Tf}] tensor")
    if tuple(rays_o.shape) != (N, 3) or tuple(rays_d.shape) != (N, 3):
        raise _lib.UcsaError("rays_o / rays_d must be [N, 3] with N = z_c.shape[0]")
    need = int(lib().ucsa_hashgrid_bwd_workspace_bytes(N, Tc + Tf, L))
    key = (z_c.device, _raw_current_stream())
    ws = _bwd_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=z_c.device)
        _bwd_ws[key] = ws
    if rec_scale > 0.0:   # half2 x rec_scale records (training modes fp16 / tcnn)
        check(lib().ucsa_hashgrid_bwd_rays_merged_h16(
            C.byref(grid), _ptr(rays_o), _ptr(rays_d), _ptr(z_c), _ptr(z_f), _ptr(src),
            fvec(aabb), N, Tc, Tf, _ptr(d_feat_c), _ptr(d_feat_f), _ptr(grad_table), _ptr(ws),
            float(rec_scale), _stream()), "ucsa_hashgrid_bwd_rays_merged_h16")
        return
    fn = lib().ucsa_hashgrid_bwd_rays_merged_p64 if packed else lib().ucsa_hashgrid_bwd_rays_merged
    check(fn(
        C.byref(grid), _ptr(rays_o), _ptr(rays_d), _ptr(z_c), _ptr(z_f), _ptr(src),
        fvec(aabb), N, Tc, Tf, _ptr(d_feat_c), _ptr(d_feat_f), _ptr(grad_table), _ptr(ws),
        _stream()), "ucsa_hashgrid_bwd_rays_merged" + ("_p64" if packed else ""))


def train_packs(sigma_x3, color_x3, sem_x3, sigma_t_x3=None, color_t_x3=None,
                sem_t_x3=None, sigma_h2=None, color_h2=None, sem_h2=None) -> "_lib.TrainPacks":
    """ucsa_train_packs over bf16x3 weight fragments (mlp_pack_x3 / mlp_pack_t_x3)
    and, optionally, f16x2 ones for the forward (mlp_pack_h2); the caller keeps
    the tensors alive."""
    return _lib.TrainPacks(*[_ptr(x) for x in (sigma_x3, color_x3, sem_x3, sigma_t_x3,
                                              color_t_x3, sem_t_x3, sigma_h2, color_h2,
                                              sem_h2)])


def render_fused_fwd(grid: Grid, table, packs, rays_o, rays_d, norms, aabb,
                     min_near: float, t_rand, u, T: int, t: int, n_classes: int,
                     density_scale: float = 1.0):
    """The training forward (rows a2-a9) as ONE C call (ucsa_render_fused_fwd,
    bf16x3 nets) -> image [N,3], depth [N], sem [N,C] and the dict of saved
    tensors (the members of ucsa_train_buffers) the fused backward reads."""
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    norms = _f32(norms, "norms").view(-1)
    N, dev, L = rays_o.shape[0], rays_o.device, grid.n_levels
    if t_rand is not None:
        t_rand = _f32(t_rand, "t_rand")
        assert t_rand.shape == (N, T)
    if t > 0:
        u = _f32(u, "u")
        assert u.shape == (N, t)
    e = lambda *shape, **kw: torch.empty(*shape, device=dev, **kw)  # noqa: E731
    # The saved tensors of a step are carved from ONE allocation at fixed, skewed
    # offsets (array i starts 256 * (2 i + 1) bytes past a 4 KiB boundary).  As
    # ten separate torch.empty calls their relative placement was whatever the
    # caching allocator's history made it, and the step time followed it: +0.15 ms
    # (3.40 -> 3.55 ms) after ONE extra device synchronisation earlier in the
    # process (round 5, tools/gpu notes in the notebook); the C side already
    # skews its own workspace for the same reason (render_train.hip).
    shapes = [("z_c", (N, T), 4), ("feat_c", (L, N * T, 2), 4), ("h_c", (N * T, 16), 4),
              ("sigma_c", (N, T), 4)]
    if t:
        shapes += [("z_f", (N, t), 4), ("feat_f", (L, N * t, 2), 4), ("h_f", (N * t, 16), 4),
                   ("sigma_f", (N, t), 4)]
    shapes += [("src", (N, T + t), 4), ("weights", (N, T + t), 4)]
    offs, end = [], 0
    for i, (_, shp, b) in enumerate(shapes):
        start = (end + 4095) // 4096 * 4096 + 256 * (2 * i + 1)
        n = b
        for d_ in shp:
            n *= d_
        offs.append(start)
        end = start + n
    slab = torch.empty(end + 4096, dtype=torch.uint8, device=dev)
    base = (-slab.data_ptr()) % 4096          # 4 KiB-aligned origin inside the slab
    sv = {k: None for k in ("z_f", "feat_f", "h_f", "sigma_f")}
    for (k, shp, b), off in zip(shapes, offs):
        n = b
        for d_ in shp:
            n *= d_
        raw = slab[base + off: base + off + n]
        sv[k] = raw.view(torch.int32 if k == "src" else torch.float32).view(*shp)
    bufs = _lib.TrainBuffers(*[_ptr(sv[k]) for k, _ in _lib.TrainBuffers._fields_])
    image, depth, sem = e(N, 3), e(N), e(N, n_classes)
    ws = _scratch_named("render_fused_fwd",
                        int(lib().ucsa_render_fused_fwd_workspace_bytes(N, T, t)), dev)
    aabb_h = fvec(aabb.detach().cpu().tolist() if torch.is_tensor(aabb) else aabb)
    check(lib().ucsa_render_fused_fwd(
        C.byref(grid), _ptr(table), C.byref(packs), _ptr(rays_o), _ptr(rays_d), _ptr(norms),
        aabb_h, float(min_near), _ptr(t_rand), _ptr(u) if t else None, N, T, t, n_classes,
        float(density_scale), C.byref(bufs), _ptr(image), _ptr(depth), _ptr(sem), _ptr(ws),
        _stream()), "ucsa_render_fused_fwd")
    return image, depth, sem, sv


def render_fused_bwd(grid: Grid, packs, rays_o, rays_d, norms, aabb, saved: dict,
                     d_image, d_depth, d_sem, n_classes: int, density_scale: float,
                     grad_table, grad_sigma, grad_color, grad_sem):
    """The training backward as ONE C call (ucsa_render_fused_bwd: bf16x2
    contractions, packed bin records).  ADDS to grad_table, overwrites the three
    net gradients."""
    N, T = saved["z_c"].shape
    t = 0 if saved["z_f"] is None else saved["z_f"].shape[1]
    dev = saved["z_c"].device
    d_image = _f32(d_image, "d_image").view(N, 3)
    d_depth = _f32(d_depth, "d_depth").view(N)
    d_sem = _f32(d_sem, "d_sem").view(N, n_classes)
    nsem = 1024 + 1024 * ((n_classes + 15) // 16)
    assert grad_sigma.numel() == 3072 and grad_color.numel() == 7168 and grad_sem.numel() == nsem
    bufs = _lib.TrainBuffers(*[_ptr(saved[k]) for k, _ in _lib.TrainBuffers._fields_])
    ws = _scratch_named("render_fused_bwd", int(lib().ucsa_render_fused_bwd_workspace_bytes(
        N, T, t, n_classes, grid.n_levels)), dev)
    aabb_h = fvec(aabb.detach().cpu().tolist() if torch.is_tensor(aabb) else aabb)
    check(lib().ucsa_render_fused_bwd(
        C.byref(grid), C.byref(packs), _ptr(rays_o), _ptr(rays_d), _ptr(norms), aabb_h,
        C.byref(bufs), _ptr(d_image), _ptr(d_depth), _ptr(d_sem), N, T, t, n_classes,
        float(density_scale), _ptr(grad_table), _ptr(grad_sigma), _ptr(grad_color),
        _ptr(grad_sem), _ptr(ws), _stream()), "ucsa_render_fused_bwd")


def hashgrid_bwd_points(grid: Grid, x, d_feat, grad_table, binned: bool = True):
    """Backward of hashgrid_encode_points: adds into grad_table."""
    x = _f32(x, "x").view(-1, 3)
    M = x.shape[0]
    if tuple(d_feat.shape) != (grid.n_levels, M, 2) or not d_feat.is_contiguous():
        raise _lib.UcsaError(
            f"d_feat must be a contiguous [{grid.n_levels}, {M}, 2] tensor, got "
            f"{tuple(d_feat.shape)}")
    ws = None
    if binned:
        need = int(lib().ucsa_hashgrid_bwd_workspace_bytes(M, 1, grid.n_levels))
        key = (x.device, _raw_current_stream())
        ws = _bwd_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            _bwd_ws[key] = ws
    check(lib().ucsa_hashgrid_bwd_points(C.byref(grid), _ptr(x), M,
                                         _ptr(d_feat), _ptr(grad_table),
                                         _ptr(ws), _stream()),
          "ucsa_hashgrid_bwd_points")


def mlp_pack_t_f16(kind: int, params: torch.Tensor, n_classes: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _mlp_pack("ucsa_mlp_pack_t_f16", kind, params, n_classes, out,
                     "ucsa_mlp_pack_t_f16_halves", 1, torch.float16)


def mlp_pack_t_x3(kind: int, params: torch.Tensor, n_classes: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Transposed weight fragments (dX = W^T dY) as three bf16 terms."""
    return _mlp_pack("ucsa_mlp_pack_t_x3", kind, params, n_classes, out,
                     "ucsa_mlp_pack_t_x3_bytes", 2, torch.bfloat16)


def shade_bwd_split() -> bool:
    """The colour / semantics backward runs as the per-net kernel pair
    (default; UCSA_SHADE_BWD_SPLIT=0 keeps the single kernel)."""
    return os.environ.get("UCSA_SHADE_BWD_SPLIT", "1")[:1] != "0"


def composite_bwd(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f, src,
                  weights, packed_color, packed_sem, packed_color_t,
                  packed_sem_t, d_image, d_depth, d_sem, n_classes: int,
                  density_scale: float = 1.0, half: bool = False,
                  f16_scale: float = 1024.0, x2: bool = False):
    """-> d_h_c [N*T,16], d_h_f [N*t,16] | None, partial_color, partial_sem.
    half=True: packed weights from mlp_pack_f16 / mlp_pack_t_f16; x2=True:
    from mlp_pack_x3 / mlp_pack_t_x3 (bf16x2 contractions)."""
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    dev = z_c.device
    d_image = _f32(d_image, "d_image").view(N, 3)
    d_depth = _f32(d_depth, "d_depth").view(N)
    d_sem = _f32(d_sem, "d_sem").view(N, n_classes)
    G = torch.empty(N, T + t, device=dev)
    d_h_c = torch.empty(N * T, 16, device=dev)
    d_h_f = torch.empty(N * t, 16, device=dev) if t else None
    parts = int((lib().ucsa_composite_bwd_parts_f16 if half
                 else lib().ucsa_composite_bwd_parts)(N))
    nrb = (n_classes + 15) // 16
    pc = torch.empty(parts, 7168, device=dev)
    ps = torch.empty(parts, 1024 + 1024 * nrb, device=dev)
    head = (_ptr(rays_d), _ptr(norms), _ptr(z_c), _ptr(sigma_c), _ptr(h_c),
            _ptr(z_f), _ptr(sigma_f), _ptr(h_f), _ptr(src), _ptr(weights),
            _ptr(packed_color), _ptr(packed_sem), _ptr(packed_color_t),
            _ptr(packed_sem_t), _ptr(d_image), _ptr(d_depth), _ptr(d_sem), N, T,
            t, n_classes, float(density_scale))
    tail = (_ptr(G), _ptr(d_h_c), _ptr(d_h_f), _ptr(pc), _ptr(ps), _stream())
    if x2:
        check(lib().ucsa_composite_bwd_x2(*head, *tail), "ucsa_composite_bwd_x2")
    elif half:
        check(lib().ucsa_composite_bwd_f16(*head, float(f16_scale), *tail),
              "ucsa_composite_bwd_f16")
    else:
        check(lib().ucsa_composite_bwd(*head, *tail), "ucsa_composite_bwd")
    return d_h_c, d_h_f, pc, ps
