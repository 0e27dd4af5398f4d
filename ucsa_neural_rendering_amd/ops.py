"""Tensor-level wrappers over the C ABI (``include/ucsa_hip.h``).

PyTorch is used for device memory and streams only: every function checks its
arguments, allocates outputs with ``torch.empty`` and enqueues the HIP kernels
on torch's current stream.  No arithmetic happens here.
"""
from __future__ import annotations

import ctypes as C
import math
import operator
import os
import threading
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import Grid, check, fvec, lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_current_stream() -> int:
    if _raw_stream is not None:
        return int(_raw_stream(torch.cuda.current_device()))
    return int(torch.cuda.current_stream().cuda_stream)


def _stream():
    # torch's current stream on the current device; the raw getter is ~20x
    # cheaper than torch.cuda.current_stream() (a training step makes ~17 calls)
    return C.c_void_p(_raw_current_stream())


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.UcsaError(
            f"{name} must live on the GPU: the HIP path has no CPU fallback")
    if t.device.index != torch.cuda.current_device():
        # kernels are enqueued on the CURRENT device's current stream
        raise _lib.UcsaError(
            f"{name} is on {t.device} but the current device is cuda:"
            f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def get_rays(poses: torch.Tensor, intrinsics, H: int, W: int,
             inds: Optional[torch.Tensor] = None):
    """-> rays_o, rays_d [B,n,3], direction_norms [B,n,1]."""
    poses = _f32(poses, "poses")
    B = poses.shape[0]
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    if inds is not None:
        inds = inds.reshape(-1).to(torch.int64).contiguous()
        n = inds.numel()
    else:
        n = H * W
    o = torch.empty(B, n, 3, device=poses.device)
    d = torch.empty(B, n, 3, device=poses.device)
    nr = torch.empty(B, n, 1, device=poses.device)
    check(lib().ucsa_get_rays(_ptr(poses), B, fx, fy, cx, cy, H, W,
                              _ptr(inds), n, _ptr(o), _ptr(d), _ptr(nr),
                              _stream()), "ucsa_get_rays")
    return o, d, nr


def tile_order(inds: torch.Tensor, W: int, tile: int = 16,
               H: Optional[int] = None) -> torch.Tensor:
    """The same pixel indices (duplicates kept), ordered tile by tile
    (``tile`` x ``tile`` pixels, row-major inside a tile).  A training batch
    is a random subset of one image; with neighbouring pixels next to each
    other the 32 rays of a hash-grid-backward workgroup share their coarse
    cells (k_hashgrid_bwd<true>: 0.86 -> 0.37 ms per pass, the step 7.9 ->
    6.9 ms).  The loss is a mean over the batch, so the order is free.

    GPU batches of <= 8192 indices: one launch (``ucsa_tile_order``, LDS
    bitonic sort of the 32-bit tile keys); otherwise torch ops (the key is a
    bijection of the pixel index, so both give the same result)."""
    flat = inds.reshape(-1)
    if flat.is_cuda and flat.dtype == torch.int64 and 0 < flat.numel() <= 8192:
        flat = flat.contiguous()
        out = torch.empty_like(flat)
        # H only bounds the key range; any image containing the indices will do
        rows = int(H) if H is not None else min((0x7FFFFFFE // int(W)) // 2, 1 << 20)
        check(lib().ucsa_tile_order(_ptr(flat), flat.numel(), rows, int(W),
                                    int(tile), _ptr(out), _stream()),
              "ucsa_tile_order")
        return out.reshape(inds.shape)
    y, x = flat // W, flat % W
    key = ((y // tile) * ((W + tile - 1) // tile) + x // tile) * (tile * tile) \
        + (y % tile) * tile + x % tile
    return flat[torch.argsort(key)].reshape(inds.shape)


def near_far_from_aabb(rays_o, rays_d, aabb, min_near: float = 0.2):
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    N = rays_o.shape[0]
    aabb_h = fvec(aabb.detach().cpu().tolist() if torch.is_tensor(aabb) else aabb)
    nears = torch.empty(N, device=rays_o.device)
    fars = torch.empty(N, device=rays_o.device)
    check(lib().ucsa_near_far_from_aabb(_ptr(rays_o), _ptr(rays_d), aabb_h, N,
                                        float(min_near), _ptr(nears),
                                        _ptr(fars), _stream()),
          "ucsa_near_far_from_aabb")
    return nears, fars


def sample_coarse(nears, fars, T: int, t_rand=None):
    nears = _f32(nears, "nears").view(-1)
    fars = _f32(fars, "fars").view(-1)
    N = nears.shape[0]
    if t_rand is not None:
        t_rand = _f32(t_rand, "t_rand")
        assert t_rand.shape == (N, T)
    z = torch.empty(N, T, device=nears.device)
    check(lib().ucsa_sample_coarse(_ptr(nears), _ptr(fars), _ptr(t_rand), N, T,
                                   _ptr(z), _stream()), "ucsa_sample_coarse")
    return z


def hashgrid_encode_rays(grid: Grid, table, rays_o, rays_d, z, aabb,
                         image_width: int = 0, half_features: bool = False):
    """-> feat [L, N*T, 2] (level-major).  image_width > 0: the rays are the
    pixels of full image rows (tile-ordered gather, same result).  An fp16
    table (table_to_half) or half_features=True gives fp16 features (for
    sigma_mlp_fwd_f16)."""
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    z = _f32(z, "z")
    N, T = z.shape
    if table.dtype == torch.float16:   # fp16 table (table_to_half) -> fp16 features
        feat = torch.empty(grid.n_levels, N * T, 2, dtype=torch.float16,
                           device=z.device)
        check(lib().ucsa_hashgrid_encode_rays_h16(
            C.byref(grid), _ptr(table), _ptr(rays_o), _ptr(rays_d), _ptr(z),
            fvec(aabb), N, T, int(image_width), _ptr(feat), _stream()),
            "ucsa_hashgrid_encode_rays_h16")
        return feat
    if half_features:
        feat = torch.empty(grid.n_levels, N * T, 2, dtype=torch.float16,
                           device=z.device)
        check(lib().ucsa_hashgrid_encode_rays_hf(
            C.byref(grid), _ptr(table), _ptr(rays_o), _ptr(rays_d), _ptr(z),
            fvec(aabb), N, T, int(image_width), _ptr(feat), _stream()),
            "ucsa_hashgrid_encode_rays_hf")
        return feat
    feat = torch.empty(grid.n_levels, N * T, 2, device=z.device)
    if image_width:
        check(lib().ucsa_hashgrid_encode_rays_image(
            C.byref(grid), _ptr(table), _ptr(rays_o), _ptr(rays_d), _ptr(z),
            fvec(aabb), N, T, int(image_width), _ptr(feat), _stream()),
            "ucsa_hashgrid_encode_rays_image")
        return feat
    check(lib().ucsa_hashgrid_encode_rays(C.byref(grid), _ptr(table),
                                          _ptr(rays_o), _ptr(rays_d), _ptr(z),
                                          fvec(aabb), N, T, _ptr(feat),
                                          _stream()),
          "ucsa_hashgrid_encode_rays")
    return feat


def tile_depth_order(z, image_width: int):
    """z [N,T] of image-ordered rays (whole rows, N % image_width == 0) ->
    (z_sorted [N*T] f32, pix [N*T] u8, slot [N*T] int32): every 8x8 pixel
    tile's samples in depth order, tiles back to back; ``slot`` = the ray-major
    index r * T + s of each (ucsa_tile_depth_order)."""
    z = _f32(z, "z")
    N, T = z.shape
    z_sorted = torch.empty(N * T, device=z.device)
    pix = torch.empty(N * T, dtype=torch.uint8, device=z.device)
    slot = torch.empty(N * T, dtype=torch.int32, device=z.device)
    check(lib().ucsa_tile_depth_order(_ptr(z), N, T, int(image_width), _ptr(z_sorted),
                                      _ptr(pix), _ptr(slot), _stream()),
          "ucsa_tile_depth_order")
    return z_sorted, pix, slot


def tile_index_order(z, image_width: int):
    """The arrays of ``tile_depth_order`` for COARSE samples without a sort: every
    8x8 tile's samples ordered by (sample index, pixel) (ucsa_tile_index_order)."""
    z = _f32(z, "z")
    N, T = z.shape
    z_sorted = torch.empty(N * T, device=z.device)
    pix = torch.empty(N * T, dtype=torch.uint8, device=z.device)
    slot = torch.empty(N * T, dtype=torch.int32, device=z.device)
    check(lib().ucsa_tile_index_order(_ptr(z), N, T, int(image_width), _ptr(z_sorted),
                                      _ptr(pix), _ptr(slot), _stream()),
          "ucsa_tile_index_order")
    return z_sorted, pix, slot


def hashgrid_encode_sorted(grid: Grid, table, rays_o, rays_d, z_sorted, pix, aabb,
                           T: int, image_width: int, half_features: bool = False):
    """-> feat [L, N*T, 2] in the order of ``tile_depth_order`` (fp32 table)."""
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    N = rays_o.shape[0]
    z_sorted = _f32(z_sorted, "z_sorted")
    if z_sorted.numel() != N * T or pix.numel() != N * T or pix.dtype != torch.uint8:
        raise UcsaError("hashgrid_encode_sorted: z_sorted / pix must hold N*T entries (pix uint8)")
    feat = torch.empty(grid.n_levels, N * T, 2, device=z_sorted.device,
                       dtype=torch.float16 if half_features else torch.float32)
    fn = (lib().ucsa_hashgrid_encode_sorted_hf if half_features
          else lib().ucsa_hashgrid_encode_sorted)
    check(fn(C.byref(grid), _ptr(table), _ptr(rays_o), _ptr(rays_d), _ptr(z_sorted),
             _ptr(pix), fvec(aabb), N, int(T), int(image_width), _ptr(feat), _stream()),
          "ucsa_hashgrid_encode_sorted")
    return feat


def sigma_mlp_fwd_scatter(mode: int, feat, packed_sigma, slot):
    """The sigma MLP (mode 0 f32-input MFMA, 1 f16 nets on fp16 features,
    2 bf16x3, 3 f16x2) on a depth-ordered feature array; h [M,16] / sigma [M]
    land at the ray-major rows ``slot``."""
    L, M, _ = feat.shape
    if slot.numel() != M or slot.dtype != torch.int32:
        raise UcsaError("sigma_mlp_fwd_scatter: slot must be int32 [M]")
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    check(lib().ucsa_sigma_mlp_fwd_scatter(int(mode), _ptr(feat), _ptr(packed_sigma), M, L,
                                           _ptr(slot), _ptr(h), _ptr(sigma), _stream()),
          "ucsa_sigma_mlp_fwd_scatter")
    return h, sigma


def density_sorted(mode: int, grid: Grid, table, rays_o, rays_d, z_sorted, pix, slot,
                   aabb, T: int, image_width: int, packed_sigma):
    """hashgrid_encode_sorted + sigma_mlp_fwd_scatter in one call, levels 0-7
    encoded inside the sigma MLP (ucsa_density_sorted; mode 2 bf16x3, 3 f16x2)
    -> h [N*T,16], sigma [N*T] at the ray-major rows."""
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    N = rays_o.shape[0]
    M = N * int(T)
    if z_sorted.numel() != M or pix.numel() != M or slot.numel() != M:
        raise _lib.UcsaError("density_sorted: z_sorted / pix / slot must hold N*T entries")
    feat_ws = torch.empty(grid.n_levels, M, 2, device=z_sorted.device)
    h = torch.empty(M, 16, device=z_sorted.device)
    sigma = torch.empty(M, device=z_sorted.device)
    check(lib().ucsa_density_sorted(
        int(mode), C.byref(grid), _ptr(table), _ptr(rays_o), _ptr(rays_d), _ptr(z_sorted),
        _ptr(pix), _ptr(slot), fvec(aabb), N, int(T), int(image_width), _ptr(packed_sigma),
        _ptr(feat_ws), _ptr(h), _ptr(sigma), _stream()), "ucsa_density_sorted")
    return h, sigma


def env_reload():
    """Make the library re-read its UCSA_* tuning switches (it snapshots them once
    per process: INTEGRATION.md "Environment variables").  Lab tools and tests
    that flip a switch inside one process call this after changing os.environ."""
    lib().ucsa_env_reload()


def hashgrid_encode_points(grid: Grid, table, x):
    x = _f32(x, "x").view(-1, 3)
    M = x.shape[0]
    feat = torch.empty(grid.n_levels, M, 2, device=x.device)
    check(lib().ucsa_hashgrid_encode_points(C.byref(grid), _ptr(table), _ptr(x),
                                            M, _ptr(feat), _stream()),
          "ucsa_hashgrid_encode_points")
    return feat


def mlp_pack(kind: int, params: torch.Tensor, n_classes: int = 0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    params = _f32(params.detach(), "params")
    if out is None:
        out = torch.empty_like(params)
    check(lib().ucsa_mlp_pack(kind, _ptr(params), _ptr(out), n_classes,
                              _stream()), "ucsa_mlp_pack")
    return out


def sigma_mlp_fwd(feat, packed_sigma) -> Tuple[torch.Tensor, torch.Tensor]:
    """feat [L,M,2] -> h [M,16], sigma [M]."""
    L, M, _ = feat.shape
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    check(lib().ucsa_sigma_mlp_fwd(_ptr(feat), _ptr(packed_sigma), M, L,
                                   _ptr(h), _ptr(sigma), _stream()),
          "ucsa_sigma_mlp_fwd")
    return h, sigma


def resample(z, sigma, u, density_scale: float = 1.0):
    """z, sigma [N, T], u [N, t] in [0, 1) -> new_z [N, t], ascending per ray
    (``ucsa_resample``).  3 <= T <= 4096, t <= 4096, and one workgroup's LDS
    must hold the rays of four waves: ``16 * (3 * T + tpad)`` bytes with
    ``tpad`` the next power of two >= t, at most 163,840 on gfx950 (T = t =
    2048 fits).  Anything larger raises ``UcsaError`` with the argument code of
    T (-1004) or t (-1005); nothing is launched."""
    z = _f32(z, "z")
    sigma = _f32(sigma, "sigma")
    u = _f32(u, "u")
    N, T = z.shape
    t = u.shape[1]
    new_z = torch.empty(N, t, device=z.device)
    check(lib().ucsa_resample(_ptr(z), _ptr(sigma), _ptr(u), N, T, t,
                              float(density_scale), _ptr(new_z), _stream()),
          "ucsa_resample")
    return new_z


def composite_fwd(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                  packed_color, packed_sem, n_classes: int,
                  density_scale: float = 1.0, want_aux: bool = False,
                  half: bool = False):
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    norms = _f32(norms, "norms").view(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    dev = z_c.device
    image = torch.empty(N, 3, device=dev)
    depth = torch.empty(N, device=dev)
    sem = torch.empty(N, n_classes, device=dev)
    src = torch.empty(N, T + t, dtype=torch.int32, device=dev) if want_aux else None
    w = torch.empty(N, T + t, device=dev) if want_aux else None
    fn = lib().ucsa_composite_fwd_f16 if half else lib().ucsa_composite_fwd
    check(fn(_ptr(rays_d), _ptr(norms), _ptr(z_c), _ptr(sigma_c), _ptr(h_c),
             _ptr(z_f), _ptr(sigma_f), _ptr(h_f), _ptr(packed_color),
             _ptr(packed_sem), N, T, t, n_classes, float(density_scale),
             _ptr(image), _ptr(depth), _ptr(sem), _ptr(src), _ptr(w), _stream()),
          "ucsa_composite_fwd")
    if want_aux:
        return image, depth, sem, src, w
    return image, depth, sem


def composite_train_fwd_x3(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                           packed_color_x3, packed_sem_x3, n_classes: int,
                           density_scale: float = 1.0, h2: bool = False):
    """Training forward of the colour / semantics stage on the split pair with
    the bf16x3 nets -> (image, depth, sem, src, w) like
    composite_fwd(want_aux=True)."""
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    norms = _f32(norms, "norms").view(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    dev = z_c.device
    image = torch.empty(N, 3, device=dev)
    depth = torch.empty(N, device=dev)
    sem = torch.empty(N, n_classes, device=dev)
    src = torch.empty(N, T + t, dtype=torch.int32, device=dev)
    w = torch.empty(N, T + t, device=dev)
    ws = _scratch_named("composite_infer",
                        int(lib().ucsa_composite_infer_workspace_bytes(N, T, t)),
                        dev)
    fn = lib().ucsa_composite_train_fwd_h2 if h2 else lib().ucsa_composite_train_fwd_x3
    check(fn(
        _ptr(rays_d), _ptr(norms), _ptr(z_c), _ptr(sigma_c), _ptr(h_c), _ptr(z_f),
        _ptr(sigma_f), _ptr(h_f), _ptr(packed_color_x3), _ptr(packed_sem_x3), N, T,
        t, n_classes, float(density_scale), _ptr(image), _ptr(depth), _ptr(sem),
        _ptr(src), _ptr(w), _ptr(ws), _stream()), "ucsa_composite_train_fwd_x3")
    return image, depth, sem, src, w


def composite_infer(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                    packed_color, packed_sem, n_classes: int,
                    density_scale: float = 1.0, half: bool = False,
                    x3: bool = False, h2: bool = False):
    """Inference composite as the dense kernel pair (ucsa_composite_infer):
    same outputs as composite_fwd, bit for bit.  half=True: packed weights
    from mlp_pack_f16.  x3=True: bf16x3 nets (fp32-grade, weights from
    mlp_pack_x3; not bit-identical to the f32-input MFMA); h2=True: f16x2
    nets (mlp_pack_h2)."""
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    norms = _f32(norms, "norms").view(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    dev = z_c.device
    image = torch.empty(N, 3, device=dev)
    depth = torch.empty(N, device=dev)
    sem = torch.empty(N, n_classes, device=dev)
    ws = _scratch_named("composite_infer",
                        int(lib().ucsa_composite_infer_workspace_bytes(N, T, t)),
                        dev)
    fn = (lib().ucsa_composite_infer_h2 if h2 else lib().ucsa_composite_infer_x3 if x3 else
          lib().ucsa_composite_infer_f16 if half else lib().ucsa_composite_infer)
    check(fn(_ptr(rays_d), _ptr(norms), _ptr(z_c), _ptr(sigma_c), _ptr(h_c),
             _ptr(z_f), _ptr(sigma_f), _ptr(h_f), _ptr(packed_color),
             _ptr(packed_sem), N, T, t, n_classes, float(density_scale),
             _ptr(image), _ptr(depth), _ptr(sem), _ptr(ws), _stream()),
          "ucsa_composite_infer")
    return image, depth, sem


def point_shade(dirs, geo_feat, mask, packed_color, packed_sem, n_classes: int,
                want_rgb: bool = True, want_probs: bool = True):
    geo_feat = _f32(geo_feat, "geo_feat").view(-1, 15)
    M = geo_feat.shape[0]
    dev = geo_feat.device
    dirs = None if dirs is None else _f32(dirs, "d").view(M, 3)
    m8 = None if mask is None else mask.reshape(M).to(torch.uint8).contiguous()
    rgb = torch.empty(M, 3, device=dev) if want_rgb else None
    probs = torch.empty(M, n_classes, device=dev) if want_probs else None
    check(lib().ucsa_point_shade(_ptr(dirs), _ptr(geo_feat), _ptr(m8),
                                 _ptr(packed_color), _ptr(packed_sem), M,
                                 n_classes, _ptr(rgb), _ptr(probs), _stream()),
          "ucsa_point_shade")
    return rgb, probs


def point_shade_h(dirs, h, packed_color, packed_sem, n_classes: int,
                  rgb=None, probs=None):
    """colour + semantics of M points straight from the sigma-MLP rows
    h [M,16]; optional preallocated outputs."""
    M = h.shape[0]
    dev = h.device
    dirs = _f32(dirs, "d").view(-1, 3)
    if rgb is None:
        rgb = torch.empty(M, 3, device=dev)
    if probs is None:
        probs = torch.empty(M, n_classes, device=dev)
    check(lib().ucsa_point_shade_h(_ptr(dirs), _ptr(h), None,
                                   _ptr(packed_color), _ptr(packed_sem), M,
                                   n_classes, _ptr(rgb), _ptr(probs),
                                   _stream()), "ucsa_point_shade_h")
    return rgb, probs


def render_workspace_bytes(N: int, T: int, t: int, n_levels: int) -> int:
    return int(lib().ucsa_render_workspace_bytes(N, T, t, n_levels))


def render_fwd(grid: Grid, table, packed_sigma, packed_color, packed_sem,
               rays_o, rays_d, norms, aabb, min_near: float, t_rand, u, T: int,
               t: int, n_classes: int, density_scale: float, image, depth,
               semantics, ws: torch.Tensor, image_width: int = 0):
    """All tensors already validated/contiguous; outputs written in place.
    image_width > 0: the rays are the pixels of full image rows."""
    N = rays_o.shape[0]
    check(lib().ucsa_render_fwd(C.byref(grid), _ptr(table), _ptr(packed_sigma),
                                _ptr(packed_color), _ptr(packed_sem),
                                _ptr(rays_o), _ptr(rays_d), _ptr(norms),
                                fvec(aabb), float(min_near), _ptr(t_rand),
                                _ptr(u), N, T, t, n_classes,
                                float(density_scale), int(image_width),
                                _ptr(image), _ptr(depth), _ptr(semantics),
                                _ptr(ws), _stream()),
          "ucsa_render_fwd")


# ======================= fp16-MFMA inference option =========================
def mlp_pack_f16(kind: int, params: torch.Tensor, n_classes: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_f16_halves(kind, n_classes))
    if out is None:
        out = torch.empty(n, dtype=torch.float16, device=params.device)
    check(lib().ucsa_mlp_pack_f16(kind, _ptr(params), _ptr(out), n_classes,
                                  _stream()), "ucsa_mlp_pack_f16")
    return out


def mlp_pack_x3(kind: int, params: torch.Tensor, n_classes: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weights as three bf16 terms per value in MFMA fragment order
    (csrc/mfma_mlp_x3.h)."""
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_x3_bytes(kind, n_classes))
    if out is None:
        out = torch.empty(n // 2, dtype=torch.bfloat16, device=params.device)
    check(lib().ucsa_mlp_pack_x3(kind, _ptr(params), _ptr(out), n_classes,
                                 _stream()), "ucsa_mlp_pack_x3")
    return out


def mlp_pack_h2(kind: int, params: torch.Tensor, n_classes: int = 0,
                out: Optional[torch.Tensor] = None,
                range_bits: Optional[torch.Tensor] = None,
                scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weights as two f16 terms per value (the second scaled by 2^11) in MFMA
    fragment order (csrc/mfma_mlp_h2.h, "f16x2").  ``range_bits`` (int32 [1] in
    pinned host or device memory, zeroed by the caller) accumulates the largest
    |value| converted to f16 as an fp32 bit pattern; ``scratch``: int32 [2] on
    the device, zeroed once (ucsa_mlp_pack_h2_checked)."""
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_h2_bytes(kind, n_classes))
    if out is None:
        out = torch.empty(n // 2, dtype=torch.float16, device=params.device)
    if range_bits is not None:
        if scratch is None or not scratch.is_cuda or scratch.numel() < 2:
            raise UcsaError("mlp_pack_h2: range_bits needs a 2-word int32 device scratch")
        check(lib().ucsa_mlp_pack_h2_checked(kind, _ptr(params), _ptr(out), n_classes,
                                             _ptr(range_bits), _ptr(scratch), _stream()),
              "ucsa_mlp_pack_h2_checked")
        return out
    check(lib().ucsa_mlp_pack_h2(kind, _ptr(params), _ptr(out), n_classes,
                                 _stream()), "ucsa_mlp_pack_h2")
    return out


def sigma_mlp_fwd_h2(feat, packed_sigma_h2):
    L, M, _ = feat.shape
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    check(lib().ucsa_sigma_mlp_fwd_h2(_ptr(feat), _ptr(packed_sigma_h2), M, L,
                                      _ptr(h), _ptr(sigma), _stream()),
          "ucsa_sigma_mlp_fwd_h2")
    return h, sigma


def render_fwd_h2(grid: Grid, table, packed_sigma_h2, packed_color_h2,
                  packed_sem_h2, rays_o, rays_d, norms, aabb, min_near: float,
                  t_rand, u, T: int, t: int, n_classes: int,
                  density_scale: float, image, depth, semantics,
                  ws: torch.Tensor, image_width: int = 0):
    """run() with the three nets as f16x2 (fp32-grade on the f16 MFMA pipe,
    three passes per product)."""
    N = rays_o.shape[0]
    check(lib().ucsa_render_fwd_h2(
        C.byref(grid), _ptr(table), _ptr(packed_sigma_h2), _ptr(packed_color_h2),
        _ptr(packed_sem_h2), _ptr(rays_o), _ptr(rays_d), _ptr(norms), fvec(aabb),
        float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws), _stream()), "ucsa_render_fwd_h2")


def sigma_mlp_fwd_f16(feat, packed_sigma_half):
    L, M, _ = feat.shape
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    if feat.dtype == torch.float16:   # features of the fp16-table encoder
        check(lib().ucsa_sigma_mlp_fwd_f16_h(_ptr(feat), _ptr(packed_sigma_half),
                                             M, L, _ptr(h), _ptr(sigma),
                                             _stream()), "ucsa_sigma_mlp_fwd_f16_h")
        return h, sigma
    check(lib().ucsa_sigma_mlp_fwd_f16(_ptr(feat), _ptr(packed_sigma_half), M,
                                       L, _ptr(h), _ptr(sigma), _stream()),
          "ucsa_sigma_mlp_fwd_f16")
    return h, sigma


def render_fwd_f16(grid: Grid, table, packed_sigma_h, packed_color_h,
                   packed_sem_h, rays_o, rays_d, norms, aabb, min_near: float,
                   t_rand, u, T: int, t: int, n_classes: int,
                   density_scale: float, image, depth, semantics,
                   ws: torch.Tensor, image_width: int = 0):
    N = rays_o.shape[0]
    check(lib().ucsa_render_fwd_f16(
        C.byref(grid), _ptr(table), _ptr(packed_sigma_h), _ptr(packed_color_h),
        _ptr(packed_sem_h), _ptr(rays_o), _ptr(rays_d), _ptr(norms), fvec(aabb),
        float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws), _stream()), "ucsa_render_fwd_f16")


def table_to_half(table: torch.Tensor, out: Optional[torch.Tensor] = None):
    """fp32 hash table -> the fp16 copy the *_h16 entry points read."""
    table = _f32(table.detach(), "table")
    if out is None:
        out = torch.empty(table.numel(), dtype=torch.float16, device=table.device)
    check(lib().ucsa_cast_f32_to_f16(_ptr(table), _ptr(out), table.numel(),
                                     _stream()), "ucsa_cast_f32_to_f16")
    return out


def render_fwd_f16_h16(grid: Grid, table_half, packed_sigma_h, packed_color_h,
                       packed_sem_h, rays_o, rays_d, norms, aabb, min_near: float,
                       t_rand, u, T: int, t: int, n_classes: int,
                       density_scale: float, image, depth, semantics,
                       ws: torch.Tensor, image_width: int = 0):
    """render_fwd_f16 reading the fp16 table (table_to_half)."""
    N = rays_o.shape[0]
    assert table_half.dtype == torch.float16
    check(lib().ucsa_render_fwd_f16_h16(
        C.byref(grid), _ptr(table_half), _ptr(packed_sigma_h), _ptr(packed_color_h),
        _ptr(packed_sem_h), _ptr(rays_o), _ptr(rays_d), _ptr(norms), fvec(aabb),
        float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws), _stream()), "ucsa_render_fwd_f16_h16")


def sigma_mlp_fwd_x3(feat, packed_sigma_x3):
    L, M, _ = feat.shape
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    check(lib().ucsa_sigma_mlp_fwd_x3(_ptr(feat), _ptr(packed_sigma_x3), M, L,
                                      _ptr(h), _ptr(sigma), _stream()),
          "ucsa_sigma_mlp_fwd_x3")
    return h, sigma


def render_fwd_x3(grid: Grid, table, packed_sigma_x3, packed_color_x3,
                  packed_sem_x3, rays_o, rays_d, norms, aabb, min_near: float,
                  t_rand, u, T: int, t: int, n_classes: int,
                  density_scale: float, image, depth, semantics,
                  ws: torch.Tensor, image_width: int = 0):
    """run() with the three nets as bf16x3 (fp32-grade on the bf16 MFMA pipe)."""
    N = rays_o.shape[0]
    check(lib().ucsa_render_fwd_x3(
        C.byref(grid), _ptr(table), _ptr(packed_sigma_x3), _ptr(packed_color_x3),
        _ptr(packed_sem_x3), _ptr(rays_o), _ptr(rays_d), _ptr(norms), fvec(aabb),
        float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws), _stream()), "ucsa_render_fwd_x3")


RENDER_MODES = {"fp32": 0, "fp16": 1, "bf16x3": 2, "fp16_h16": 3, "f16x2": 4}


def render_view(mode: str, grid: Grid, table, packed_sigma, packed_color, packed_sem,
                rays_o, rays_d, norms, aabb, min_near: float, t_rand, u, T: int,
                t: int, n_classes: int, density_scale: float, image, depth,
                semantics, chunk: int, ws0: torch.Tensor, ws1, image_width: int = 0):
    """All N rays in `chunk`-ray pieces as ONE call (ucsa_render_view): the
    density half of chunk k+1 overlaps the shading half of chunk k on two
    internal streams; ``ws1`` None = the serial loop.  Same bits either way."""
    N = rays_o.shape[0]
    check(lib().ucsa_render_view(
        RENDER_MODES[mode], C.byref(grid), _ptr(table), _ptr(packed_sigma),
        _ptr(packed_color), _ptr(packed_sem), _ptr(rays_o), _ptr(rays_d), _ptr(norms),
        fvec(aabb), float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), int(chunk), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws0), _ptr(ws1), _stream()), "ucsa_render_view")


# ============================ training (backward) ===========================
def mlp_pack_t(kind: int, params: torch.Tensor, n_classes: int = 0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_t_size(kind, n_classes))
    if out is None:
        out = torch.empty(n, device=params.device)
    check(lib().ucsa_mlp_pack_t(kind, _ptr(params), _ptr(out), n_classes,
                                _stream()), "ucsa_mlp_pack_t")
    return out


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
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_t_f16_halves(kind, n_classes))
    if out is None:
        out = torch.empty(n, dtype=torch.float16, device=params.device)
    check(lib().ucsa_mlp_pack_t_f16(kind, _ptr(params), _ptr(out), n_classes,
                                    _stream()), "ucsa_mlp_pack_t_f16")
    return out


def mlp_pack_t_x3(kind: int, params: torch.Tensor, n_classes: int = 0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Transposed weight fragments (dX = W^T dY) as three bf16 terms."""
    params = _f32(params.detach(), "params")
    n = int(lib().ucsa_mlp_pack_t_x3_bytes(kind, n_classes))
    if out is None:
        out = torch.empty(n // 2, dtype=torch.bfloat16, device=params.device)
    check(lib().ucsa_mlp_pack_t_x3(kind, _ptr(params), _ptr(out), n_classes,
                                   _stream()), "ucsa_mlp_pack_t_x3")
    return out


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


# ---------------------------------------------------------------------------
# occupancy-grid ray marching
# ---------------------------------------------------------------------------
def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.UcsaError(
            f"{name} must live on the GPU: the HIP path has no CPU fallback")
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise _lib.UcsaError(f"{name} must be a contiguous int32 tensor")
    return t


def _inplace_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.UcsaError(
            f"{name} is updated in place: contiguous fp32 on the GPU required")
    return t


_march_ws = {}
_named_ws = {}


def _scratch_named(name: str, nbytes: int, device) -> torch.Tensor:
    """A grow-only scratch buffer of its own (not shared with _scratch's).
    Keyed by the calling THREAD as well as device and stream: the
    multi-launch ops (BatchNorm: stats -> finalize -> apply; augmentation: grey
    sums -> apply) pass intermediates through it, ctypes releases the GIL, and the
    trainer's prefetch thread issues on the same stream as the training step -- two
    threads sharing one buffer would overwrite each other's partial sums."""
    key = (name, device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    buf = _named_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _named_ws[key] = buf
    return buf


def _scratch(nbytes: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    buf = _march_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8,
                          device=device)
        _march_ws[key] = buf
    return buf


def march_rays_train(rays_o, rays_d, density_grid, mean_density: float,
                     bound: float, dt_gamma: float, M: int, nears, fars, xyzs,
                     dirs, deltas, rays, counter, perturb: int):
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    grid = _f32(density_grid, "density_grid")
    N, Cc, H = rays_o.shape[0], grid.shape[0], grid.shape[1]
    ws = _scratch(int(lib().ucsa_march_workspace_bytes(N)), rays_o.device)
    check(lib().ucsa_march_rays_train(
        _ptr(rays_o), _ptr(rays_d), _ptr(grid), mean_density, bound, dt_gamma,
        N, Cc, H, M, _ptr(_f32(nears, "nears")), _ptr(_f32(fars, "fars")),
        _ptr(xyzs), _ptr(dirs), _ptr(deltas), _ptr(_i32(rays, "rays")),
        _ptr(_i32(counter, "step_counter")), int(perturb), _ptr(ws),
        _stream()), "ucsa_march_rays_train")


def composite_rays_train_fwd(sigmas, rgbs, local_sem, deltas, rays):
    sigmas = _f32(sigmas, "sigmas").view(-1)
    M, N = sigmas.shape[0], rays.shape[0]
    rgbs = _f32(rgbs, "rgbs").view(M, 3)
    deltas = _f32(deltas, "deltas").view(M, 2)
    dev = sigmas.device
    n_sem = 0
    if local_sem is not None:
        local_sem = _f32(local_sem, "local_semantics").view(M, -1)
        n_sem = local_sem.shape[1]
    ws = torch.empty(N, device=dev)
    depth = torch.empty(N, device=dev)
    image = torch.empty(N, 3, device=dev)
    sem = torch.empty(N, n_sem, device=dev) if n_sem else None
    check(lib().ucsa_composite_rays_train_fwd(
        _ptr(sigmas), _ptr(rgbs), _ptr(local_sem), _ptr(deltas),
        _ptr(_i32(rays, "rays")), M, N, n_sem, _ptr(ws), _ptr(depth),
        _ptr(image), _ptr(sem), _stream()), "ucsa_composite_rays_train_fwd")
    return ws, depth, image, sem


def composite_rays_train_bwd(grad_ws, grad_image, grad_sem, sigmas, rgbs,
                             deltas, rays, weights_sum, image):
    M, N = sigmas.shape[0], rays.shape[0]
    dev = sigmas.device
    n_sem = 0 if grad_sem is None else grad_sem.shape[1]
    g_sig = torch.zeros(M, device=dev)
    g_rgb = torch.zeros(M, 3, device=dev)
    g_ls = torch.zeros(M, n_sem, device=dev) if n_sem else None
    check(lib().ucsa_composite_rays_train_bwd(
        _ptr(_f32(grad_ws, "grad_weights_sum")),
        _ptr(_f32(grad_image, "grad_image")),
        _ptr(None if grad_sem is None else _f32(grad_sem, "grad_semantics")),
        _ptr(sigmas), _ptr(rgbs), _ptr(deltas), _ptr(rays), _ptr(weights_sum),
        _ptr(image), M, N, n_sem, _ptr(g_sig), _ptr(g_rgb), _ptr(g_ls),
        _stream()), "ucsa_composite_rays_train_bwd")
    return g_sig, g_rgb, g_ls


def march_rays(n_alive: int, n_step: int, rays_alive, rays_t, rays_o, rays_d,
               bound: float, dt_gamma: float, density_grid, mean_density: float,
               nears, fars, xyzs, dirs, deltas, perturb: int):
    rays_o = _f32(rays_o, "rays_o").view(-1, 3)
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    grid = _f32(density_grid, "density_grid")
    check(lib().ucsa_march_rays(
        n_alive, n_step, _ptr(_i32(rays_alive, "rays_alive")),
        _ptr(_f32(rays_t, "rays_t")), _ptr(rays_o), _ptr(rays_d), bound,
        dt_gamma, grid.shape[0], grid.shape[1], _ptr(grid), mean_density,
        _ptr(_f32(nears, "nears")), _ptr(_f32(fars, "fars")), _ptr(xyzs),
        _ptr(dirs), _ptr(deltas), int(perturb), _stream()), "ucsa_march_rays")


def composite_rays(n_alive: int, n_step: int, rays_alive, rays_t, sigmas, rgbs,
                   local_sem, deltas, weights_sum, depth, image, semantics):
    n_sem = 0
    if local_sem is not None:
        local_sem = _f32(local_sem, "local_semantics")
        n_sem = local_sem.shape[-1]
        _inplace_f32(semantics, "semantics")
    check(lib().ucsa_composite_rays(
        n_alive, n_step, _ptr(_i32(rays_alive, "rays_alive")),
        _ptr(_inplace_f32(rays_t, "rays_t")), _ptr(_f32(sigmas, "sigmas")),
        _ptr(_f32(rgbs, "rgbs")), _ptr(local_sem), _ptr(_f32(deltas, "deltas")),
        n_sem, _ptr(_inplace_f32(weights_sum, "weights_sum")),
        _ptr(_inplace_f32(depth, "depth")), _ptr(_inplace_f32(image, "image")),
        _ptr(semantics), _stream()), "ucsa_composite_rays")


def compact_rays(n_alive: int, rays_alive, rays_alive_old, rays_t, rays_t_old,
                 alive_counter):
    ws = _scratch(int(lib().ucsa_compact_workspace_bytes(n_alive)),
                  rays_t.device)
    check(lib().ucsa_compact_rays(
        n_alive, _ptr(_i32(rays_alive, "rays_alive")),
        _ptr(_i32(rays_alive_old, "rays_alive_old")),
        _ptr(_inplace_f32(rays_t, "rays_t")),
        _ptr(_f32(rays_t_old, "rays_t_old")),
        _ptr(_i32(alive_counter, "alive_counter")), _ptr(ws), _stream()),
        "ucsa_compact_rays")


def density_grid_points(cascade: int, H: int, bound: float, seed: int, device):
    xyz = torch.empty(H * H * H, 3, device=device)
    check(lib().ucsa_density_grid_points(cascade, H, bound, seed, _ptr(xyz),
                                         _stream()), "ucsa_density_grid_points")
    return xyz


def density_grid_update(density_grid, fresh, decay: float, fresh_scale: float):
    """In place on density_grid; returns the new mean density (device [1])."""
    _inplace_f32(density_grid, "density_grid")
    fresh = _f32(fresh, "fresh")
    n = density_grid.numel()
    mean = torch.empty(1, device=density_grid.device)
    ws = _scratch(int(lib().ucsa_density_grid_workspace_bytes()),
                  density_grid.device)
    check(lib().ucsa_density_grid_update(_ptr(density_grid), _ptr(fresh), n,
                                         decay, fresh_scale, _ptr(mean),
                                         _ptr(ws), _stream()),
          "ucsa_density_grid_update")
    return mean


class MarchSegments:
    """Buffers + calls of the segmented marcher (``ucsa_march_segment_*``) for
    one batch of N rays; see include/ucsa_hip.h."""

    def __init__(self, rays_o, rays_d, nears, fars, density_grid,
                 mean_density: float, bound: float, dt_gamma: float):
        self.o = _f32(rays_o, "rays_o").view(-1, 3)
        self.d = _f32(rays_d, "rays_d").view(-1, 3)
        self.fars = _f32(fars, "fars")
        self.grid = _f32(density_grid, "density_grid")
        self.args = (float(bound), float(dt_gamma), self.grid.shape[0],
                     self.grid.shape[1])
        self.mean_density = float(mean_density)
        N = self.o.shape[0]
        dev = self.o.device
        self.N = N
        self.alive = torch.empty(2, N, dtype=torch.int32, device=dev)
        self.alive[0] = torch.arange(N, dtype=torch.int32, device=dev)
        self.t = torch.empty(2, N, device=dev)
        self.t[0] = _f32(nears, "nears")
        self.span = torch.empty(N, 2, dtype=torch.int32, device=dev)
        self.n_alive = torch.empty(2, dtype=torch.int32, device=dev)
        self.ws = torch.empty(
            int(lib().ucsa_march_segment_workspace_bytes(N)) // 4,
            dtype=torch.int32, device=dev)
        self.cur = 0        # which half of alive / t / n_alive is current
        self.first = True   # round 0: every ray alive, count not on device yet
        self.stage = None   # staging rows of the current round (or None)
        self.stage_cap = 0
        # rounds whose staging rows fit this many bytes march once (the
        # samples are staged while counting, then copied into place)
        self.stage_limit = 1 << 30

    def _n_dev(self):
        return None if self.first else _ptr(self.n_alive[self.cur:])

    def count(self, n_cap: int, cap: int, perturb: int):
        b, g, C_, H = self.args
        need = int(lib().ucsa_march_segment_stage_bytes(n_cap, cap))
        self.stage, self.stage_cap = None, cap
        if 0 < need <= self.stage_limit:
            self.stage = _scratch_named("march_stage", need, self.o.device)
        check(lib().ucsa_march_segment_count(
            n_cap, self._n_dev(), cap, _ptr(self.alive[self.cur]),
            _ptr(self.t[self.cur]), _ptr(self.o), _ptr(self.d), b, g, C_, H,
            _ptr(self.grid), self.mean_density, _ptr(self.fars), int(perturb),
            _ptr(self.span), _ptr(self.ws), _ptr(self.stage), _stream()),
            "ucsa_march_segment_count")
        total, n_alive = self.ws[:2].tolist()   # the round's one host sync
        return total, n_alive

    def write(self, n_cap: int, M: int, perturb: int):
        b, g, C_, H = self.args
        dev = self.o.device
        xyzs = torch.empty(M, 3, device=dev)
        dirs = torch.empty(M, 3, device=dev)
        deltas = torch.empty(M, 2, device=dev)
        check(lib().ucsa_march_segment_write(
            n_cap, self._n_dev(), _ptr(self.alive[self.cur]),
            _ptr(self.t[self.cur]), _ptr(self.o), _ptr(self.d), b, g, C_, H,
            _ptr(self.grid), self.mean_density, _ptr(self.fars), int(perturb),
            _ptr(self.span), _ptr(xyzs), _ptr(dirs), _ptr(deltas),
            _ptr(self.stage), self.stage_cap, _stream()),
            "ucsa_march_segment_write")
        return xyzs, dirs, deltas

    def composite(self, n_cap: int, cap: int, sigmas, sigma_scale: float, rgbs,
                  local_sem, deltas, weights_sum, depth, image, semantics):
        n_sem = 0 if local_sem is None else local_sem.shape[-1]
        check(lib().ucsa_march_segment_composite(
            n_cap, self._n_dev(), cap, _ptr(self.alive[self.cur]),
            _ptr(self.t[self.cur]), _ptr(self.span), _ptr(sigmas),
            float(sigma_scale), _ptr(rgbs), _ptr(local_sem), _ptr(deltas),
            n_sem, _ptr(weights_sum), _ptr(depth), _ptr(image),
            _ptr(semantics), _stream()), "ucsa_march_segment_composite")

    def shade(self, n_cap: int, cap: int, sigmas, sigma_scale: float, h,
              deltas, packed_color, packed_sem, n_classes: int, w_min: float,
              weights_sum, depth, image, semantics, half=False):
        """``half``: False -- f32-input MFMA nets (packed by mlp_pack); True / "fp16" --
        plain f16 nets (mlp_pack_f16); "f16x2" -- two-term f16 nets (mlp_pack_h2)."""
        fn = (lib().ucsa_march_segment_shade_h2 if half == "f16x2"
              else lib().ucsa_march_segment_shade_f16 if half
              else lib().ucsa_march_segment_shade)
        check(fn(n_cap, self._n_dev(), cap, _ptr(self.alive[self.cur]),
                 _ptr(self.t[self.cur]), _ptr(self.span), _ptr(self.d),
                 _ptr(sigmas), float(sigma_scale), _ptr(h), _ptr(deltas),
                 _ptr(packed_color), _ptr(packed_sem), n_classes, float(w_min),
                 _ptr(weights_sum), _ptr(depth), _ptr(image), _ptr(semantics),
                 _stream()), "ucsa_march_segment_shade")

    def compact(self, n_cap: int):
        nxt = 1 - self.cur
        check(lib().ucsa_march_segment_compact(
            n_cap, self._n_dev(), _ptr(self.alive[nxt]),
            _ptr(self.alive[self.cur]), _ptr(self.t[nxt]),
            _ptr(self.t[self.cur]), _ptr(self.n_alive[nxt:]), _ptr(self.ws),
            _stream()), "ucsa_march_segment_compact")
        self.cur = nxt
        self.first = False


def march_train_fwd(rays, M: int, nears, rays_d, sigmas, sigma_scale: float, h,
                    deltas, packed_color, packed_sem, n_classes: int,
                    w_min: float):
    """-> weights_sum [N], depth_raw [N] (sum w*t), image [N,3], sem [N,C],
    w [M], t [M]."""
    N = rays.shape[0]
    dev = rays.device
    ws = torch.zeros(N, device=dev)
    depth = torch.zeros(N, device=dev)
    image = torch.zeros(N, 3, device=dev)
    sem = torch.zeros(N, n_classes, device=dev)
    w = torch.zeros(M, device=dev)
    t = torch.zeros(M, device=dev)
    check(lib().ucsa_march_train_fwd(
        _ptr(_i32(rays, "rays")), N, M, _ptr(_f32(nears, "nears")),
        _ptr(_f32(rays_d, "rays_d")), _ptr(sigmas), float(sigma_scale), _ptr(h),
        _ptr(deltas), _ptr(packed_color), _ptr(packed_sem), n_classes,
        float(w_min), _ptr(ws), _ptr(depth), _ptr(image), _ptr(sem), _ptr(w),
        _ptr(t), _stream()), "ucsa_march_train_fwd")
    return ws, depth, image, sem, w, t


def march_train_bwd(rays, M: int, rays_d, norms, sigmas, sigma_scale: float, h,
                    deltas, w, t, packed_color, packed_sem, packed_color_t,
                    packed_sem_t, n_classes: int, w_min: float, d_image,
                    d_depth, d_sem):
    """-> d_h [M,16], partial_color, partial_sem."""
    N = rays.shape[0]
    dev = rays.device
    G = torch.empty(max(M, 1), device=dev)
    d_h = torch.empty(max(M, 1), 16, device=dev)
    parts = int(lib().ucsa_composite_bwd_parts(N))
    nrb = (n_classes + 15) // 16
    pc = torch.empty(parts, 7168, device=dev)
    ps = torch.empty(parts, 1024 + 1024 * nrb, device=dev)
    check(lib().ucsa_march_train_bwd(
        _ptr(rays), N, M, _ptr(rays_d), _ptr(norms), _ptr(sigmas),
        float(sigma_scale), _ptr(h), _ptr(deltas), _ptr(w), _ptr(t),
        _ptr(packed_color), _ptr(packed_sem), _ptr(packed_color_t),
        _ptr(packed_sem_t), n_classes, float(w_min),
        _ptr(_f32(d_image, "d_image")), _ptr(_f32(d_depth, "d_depth")),
        _ptr(_f32(d_sem, "d_sem")), _ptr(G), _ptr(d_h), _ptr(pc), _ptr(ps),
        _stream()), "ucsa_march_train_bwd")
    return d_h[:M], pc, ps


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


# ---------------------------------------------------------------------------
# marching cubes (labelled-mesh export)
# ---------------------------------------------------------------------------
def marching_cubes(field, iso: float, origin=(0.0, 0.0, 0.0),
                   spacing=(1.0, 1.0, 1.0), valid=None):
    """Indexed iso-surface of a lattice field [nx,ny,nz] (point (i,j,k) at
    origin + (i,j,k)*spacing; inside iff field > iso) ->
    (verts [V,3] f32, faces [F,3] int32, normals [V,3] f32), conventions of
    ucsa_mc_count / ucsa_mc_emit (include/ucsa_hip.h).  ``valid`` [nx,ny,nz]
    bool or uint8 (a TSDF volume's observed voxels): vertices only on edges
    between two valid points, triangles only from cells with eight valid
    corners (ucsa_mc_count_masked / ucsa_mc_emit_masked); None = every point.
    Reads the two totals back once, between the passes.  Workspace: 10 bytes
    per lattice point."""
    field = _f32(field, "field")
    if field.dim() != 3:
        raise _lib.UcsaError(f"field must be [nx,ny,nz], got {tuple(field.shape)}")
    nx, ny, nz = (int(s) for s in field.shape)
    dev = field.device
    head = (_ptr(field),)
    count, emit, what = lib().ucsa_mc_count, lib().ucsa_mc_emit, "ucsa_mc"
    if valid is not None:
        if not (torch.is_tensor(valid) and valid.is_cuda):
            raise _lib.UcsaError("valid must be a GPU tensor: the HIP path has no CPU fallback")
        if valid.dtype not in (torch.bool, torch.uint8):
            raise _lib.UcsaError(f"valid must be bool or uint8, got {valid.dtype}")
        if valid.shape != field.shape or valid.device != dev:
            raise _lib.UcsaError(f"valid must be {tuple(field.shape)} on {dev}, got "
                                 f"{tuple(valid.shape)} on {valid.device}")
        valid = valid.contiguous().view(torch.uint8)
        head = (_ptr(field), _ptr(valid))
        count, emit, what = lib().ucsa_mc_count_masked, lib().ucsa_mc_emit_masked, \
            "ucsa_mc_masked"
    ws = torch.empty(int(lib().ucsa_mc_workspace_bytes(nx, ny, nz)), dtype=torch.uint8,
                     device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    check(count(*head, nx, ny, nz, float(iso), _ptr(ws), _ptr(totals), _stream()),
          what + " count")
    V, F = (int(v) & 0xFFFFFFFF for v in totals.tolist())
    if V > 0x7FFFFFFF or F > 0x7FFFFFFF:
        raise _lib.UcsaError("marching_cubes: more than 2^31-1 vertices or triangles; "
                             "use a coarser lattice or split it")
    verts = torch.empty(V, 3, device=dev)
    normals = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V or F:
        check(emit(*head, nx, ny, nz, float(iso), fvec(origin), fvec(spacing), _ptr(ws),
                   _ptr(verts), _ptr(normals), _ptr(faces), V, F, _stream()), what + " emit")
    return verts, faces, normals


# ---------------------------------------------------------------------------
# mesh rasterization (labelled meshes into camera views)
# ---------------------------------------------------------------------------
RASTER_MAX_DIM = 16384


def rasterize_mesh(verts, faces, poses, intrinsics, H: int, W: int, near: float,
                   vertex_labels=None, vertex_rgb=None):
    """A triangle mesh seen from B pinhole cameras (poses [B,4,4]
    camera-to-world in the field's frame, intrinsics (fx, fy, cx, cy): the
    conventions of get_rays) -> dict of device tensors ``tri_id`` [B,H,W] int32
    (-1 = empty), ``depth`` [B,H,W] f32 z-depth (0 = empty), ``label`` [B,H,W]
    int32 (``vertex_labels`` of the nearest corner of the hit point, 0 = empty
    or no labels) and, with ``vertex_rgb`` [V,3], ``rgb`` [B,H,W,3] f32
    (barycentric blend).  verts [V,3] f32, faces [F,3] int32 with indices in
    [0,V).  Contract of ucsa_raster_setup / ucsa_raster_draw
    (include/ucsa_hip.h): watertight, nearest face wins, ties to the lower face
    id, deterministic.  Reads back the face index range (validation) and,
    between the passes, the (tile, face) pair total."""
    verts = _f32(verts, "verts")
    poses = _f32(poses, "poses")
    if not (torch.is_tensor(faces) and faces.is_cuda):
        raise _lib.UcsaError("faces must be a GPU tensor: the HIP path has no CPU fallback")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise _lib.UcsaError(f"faces must be an integer tensor, got {faces.dtype}")
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise _lib.UcsaError(f"verts must be [V,3], got {tuple(verts.shape)}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.UcsaError(f"faces must be [F,3], got {tuple(faces.shape)}")
    if poses.dim() != 3 or poses.shape[1:] != (4, 4) or poses.shape[0] < 1:
        raise _lib.UcsaError(f"poses must be [B,4,4], got {tuple(poses.shape)}")
    V, F, B = int(verts.shape[0]), int(faces.shape[0]), int(poses.shape[0])
    H, W = int(H), int(W)
    if not (1 <= H <= RASTER_MAX_DIM and 1 <= W <= RASTER_MAX_DIM):
        raise _lib.UcsaError(f"H, W must be in [1, {RASTER_MAX_DIM}], got {H}x{W}")
    if B > 65535 or B * F > 0x7FFFFFFF:
        raise _lib.UcsaError("rasterize_mesh: too many views x faces in one call; "
                             "render fewer views at a time")
    near = float(near)
    if not (near > 0.0 and math.isfinite(near)):
        raise _lib.UcsaError(f"near must be > 0, got {near}")
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    if not (fx > 0 and fy > 0 and all(math.isfinite(v) for v in (fx, fy, cx, cy))):
        raise _lib.UcsaError(f"intrinsics must have fx, fy > 0 and be finite, got "
                             f"{(fx, fy, cx, cy)}")
    lo_hi = torch.stack(torch.aminmax(faces)).tolist() if F else [0, 0]
    if F and (lo_hi[0] < 0 or lo_hi[1] >= V):
        raise _lib.UcsaError(f"faces index outside [0, {V})")
    faces = _i32(faces.to(torch.int32).contiguous(), "faces")
    labels = rgb_in = None
    if vertex_labels is not None:
        labels = _i32(vertex_labels.to(torch.int32).contiguous(), "vertex_labels")
        if labels.shape != (V,):
            raise _lib.UcsaError(f"vertex_labels must be [V], got {tuple(labels.shape)}")
    if vertex_rgb is not None:
        rgb_in = _f32(vertex_rgb, "vertex_rgb")
        if rgb_in.shape != (V, 3):
            raise _lib.UcsaError(f"vertex_rgb must be [V,3], got {tuple(rgb_in.shape)}")
    dev = verts.device
    args = (_ptr(verts), V, _ptr(faces), F, _ptr(poses), B, fx, fy, cx, cy, H, W, near)
    ws = torch.empty(int(lib().ucsa_raster_workspace_bytes(B, F, H, W)), dtype=torch.uint8,
                     device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().ucsa_raster_setup(*args, _ptr(ws), _ptr(total), _stream()),
          "ucsa_raster_setup")
    n_pairs = int(total.item())
    if n_pairs > 0x7FFFFFFF:
        raise _lib.UcsaError("rasterize_mesh: more than 2^31-1 (tile, face) pairs; "
                             "render fewer views at a time")
    pairs = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    out = {"tri_id": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "depth": torch.empty(B, H, W, device=dev),
           "label": torch.empty(B, H, W, dtype=torch.int32, device=dev)}
    if rgb_in is not None:
        out["rgb"] = torch.empty(B, H, W, 3, device=dev)
    check(lib().ucsa_raster_draw(*args, _ptr(labels), _ptr(rgb_in), _ptr(ws), _ptr(pairs),
                                 n_pairs, pairs.numel(), _ptr(out["tri_id"]),
                                 _ptr(out["depth"]), _ptr(out["label"]), _ptr(out.get("rgb")),
                                 B * H * W, _stream()), "ucsa_raster_draw")
    return out


# ---------------------------------------------------------------------------
# label fusion (2D label maps voted onto mesh vertices)
# ---------------------------------------------------------------------------
def _fuse_input(t, name, dtype, n):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise _lib.UcsaError(f"{name} must be a GPU tensor: the HIP path has no CPU fallback")
    if t.device.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"{name} is on {t.device} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    if t.dtype != dtype:
        raise _lib.UcsaError(f"{name} must be {dtype}, got {t.dtype}")
    if t.numel() != n:
        raise _lib.UcsaError(f"{name} has {t.numel()} elements, vertex_id has {n}")
    return t.contiguous()


def _vote_table(votes):
    if not (torch.is_tensor(votes) and votes.is_cuda and votes.dtype == torch.int64
            and votes.is_contiguous()):
        raise _lib.UcsaError("votes must be a contiguous int64 tensor on the GPU (the bits of "
                             "the uint64 table)")
    if votes.dim() != 2 or not (2 <= votes.shape[1] <= 256):
        raise _lib.UcsaError(f"votes must be [V, C+1] with 1 <= C <= 255, got "
                             f"{tuple(votes.shape)}")
    if votes.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("votes: V*(C+1) must be at most 2^31-1")
    return int(votes.shape[0]), int(votes.shape[1]) - 1


def fuse_label_votes(votes, vertex_id, pred, weight=None, mesh_depth=None, sensor_depth=None,
                     depth_tol=None, _one_atomic_per_pixel=False):
    """Pixels vote for (vertex, class) cells of ``votes`` [V, C+1] int64 (the
    bits of a uint64 table, zeroed by the caller; column 0 unused), in place;
    returns ``votes``.  ``vertex_id`` int32, any shape (the ``label`` of
    ``rasterize_mesh(..., vertex_labels=arange(1, V+1))``: 1-based, <= 0 = no
    vote), ``pred`` uint8 class ids (1..C vote), ``weight`` int32 in [0, 65535]
    or None (1 per vote), ``mesh_depth`` / ``sensor_depth`` fp32 z in scene
    units with ``depth_tol``: a pixel then votes only where sensor_depth > 0
    and |mesh_depth - sensor_depth| <= depth_tol.  All of vertex_id's size.
    Contract of ucsa_label_fuse_accumulate (include/ucsa_hip.h): integer sums,
    the same bytes whatever the order of pixels and calls."""
    V, Cn = _vote_table(votes)
    if not torch.is_tensor(vertex_id):
        raise _lib.UcsaError("vertex_id must be a GPU tensor")
    n = vertex_id.numel()
    vid = _fuse_input(vertex_id, "vertex_id", torch.int32, n)
    pr = _fuse_input(pred, "pred", torch.uint8, n)
    if n > 0x7FFFFFFF:
        raise _lib.UcsaError("fuse_label_votes: at most 2^31-1 pixels per call")
    w = None if weight is None else _fuse_input(weight, "weight", torch.int32, n)
    if (mesh_depth is None) != (sensor_depth is None):
        raise _lib.UcsaError("mesh_depth and sensor_depth come as a pair")
    md = sd = None
    tol = 0.0
    if mesh_depth is not None:
        if depth_tol is None:
            raise _lib.UcsaError("the depth gate needs depth_tol")
        tol = float(depth_tol)
        if not tol >= 0.0:
            raise _lib.UcsaError(f"depth_tol must be >= 0, got {depth_tol}")
        md = _fuse_input(mesh_depth, "mesh_depth", torch.float32, n)
        sd = _fuse_input(sensor_depth, "sensor_depth", torch.float32, n)
    elif depth_tol is not None:
        raise _lib.UcsaError("depth_tol given without mesh_depth / sensor_depth")
    row_width = int(vertex_id.shape[-1]) if vertex_id.dim() >= 2 else 0
    check(lib().ucsa_label_fuse_accumulate(
        _ptr(vid), _ptr(pr), _ptr(w), _ptr(md), _ptr(sd), tol, n, row_width, V, Cn,
        _ptr(votes), votes.numel(), 1 if _one_atomic_per_pixel else 0, _stream()),
        "ucsa_label_fuse_accumulate")
    return votes


def resolve_label_votes(votes, min_votes: int = 1):
    """``votes`` [V, C+1] -> dict of device tensors: ``label`` [V] int32 (the
    class with the largest sum, ties to the lower id, 0 where the row's total
    is below ``min_votes``), ``total`` and ``winner`` [V] int64 (the bits of
    uint64 sums; confidence = winner / total).  ucsa_label_fuse_resolve.  On a
    table filled by ``fuse_label_evidence`` the sums are evidence sums and
    ``min_votes`` is in evidence units (a confident view adds about 255)."""
    V, Cn = _vote_table(votes)
    min_votes = int(min_votes)
    if not 1 <= min_votes < 1 << 64:
        raise _lib.UcsaError(f"min_votes must be >= 1, got {min_votes}")
    dev = votes.device
    out = {"label": torch.empty(V, dtype=torch.int32, device=dev),
           "total": torch.empty(V, dtype=torch.int64, device=dev),
           "winner": torch.empty(V, dtype=torch.int64, device=dev)}
    check(lib().ucsa_label_fuse_resolve(_ptr(votes), V, Cn, min_votes, _ptr(out["label"]),
                                        _ptr(out["total"]), _ptr(out["winner"]), V,
                                        _stream()), "ucsa_label_fuse_resolve")
    return out


def log_evidence(x, from_logits: bool = False, floor_nats: float = 8.0):
    """Class beliefs ``x`` [B,C,H,W] (probabilities, or logits with
    ``from_logits``) -> evidence codes uint8 [B,H,W,C], pixel-major (the C
    codes of a pixel are C consecutive bytes, as ``accumulate_voxel_evidence``
    and ``fuse_label_evidence`` read them):
    e_c = 255 - rint(255 * min(-ln p_c, L) / L) with L = ``floor_nats``: p = 1
    gives 255, p <= e^-L gives 0.  A sum of codes over views is the clamped
    log-likelihood sum scaled by 255 / L; an all-zero row means "abstain" and
    cannot come out of a softmax over C <= 255 classes with L = 8.  Plain
    torch in fp32 on x's device (elementwise plumbing; the HIP is in the
    accumulation)."""
    if not (torch.is_tensor(x) and x.dim() == 4 and x.is_floating_point()):
        raise _lib.UcsaError("log_evidence: x must be a floating-point tensor [B,C,H,W]")
    if not 1 <= x.shape[1] <= 255:
        raise _lib.UcsaError(f"log_evidence: 1 <= C <= 255, got {x.shape[1]}")
    L = float(floor_nats)
    if not (L > 0.0 and L < float("inf")):
        raise _lib.UcsaError(f"log_evidence: floor_nats must be > 0 and finite, got {floor_nats}")
    x = x.float()
    nl = -(torch.log_softmax(x, dim=1) if from_logits else torch.log(x))
    nl = torch.nan_to_num(nl, nan=L, posinf=L, neginf=0.0).clamp_(0.0, L)
    e = 255.0 - torch.round(nl * 255.0 / L)
    return e.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def fuse_label_evidence(votes, vertex_id, scores, mesh_depth=None, sensor_depth=None,
                        depth_tol=None):
    """The soft form of ``fuse_label_votes``: pixels add their row of evidence
    codes to their vertex's row of ``votes`` [V, C+1] int64 (the same table;
    column 0 is left untouched), in place; returns ``votes``.  ``vertex_id``
    int32 [...] as for ``fuse_label_votes``, ``scores`` uint8 [..., C]
    (``log_evidence``; an all-zero row abstains), the optional depth gate as
    for ``fuse_label_votes``.  A pixel with 1 <= vertex_id <= V that passes the
    gate adds scores[pixel, c-1] to votes[vertex_id-1, c] for c = 1..C.
    ``resolve_label_votes`` reads the table as it is; its ``min_votes`` is then
    in evidence units.  Contract of ucsa_label_fuse_evidence
    (include/ucsa_hip.h): integer sums, the same bytes whatever the order of
    pixels and calls."""
    V, Cn = _vote_table(votes)
    if not torch.is_tensor(vertex_id):
        raise _lib.UcsaError("vertex_id must be a GPU tensor")
    n = vertex_id.numel()
    vid = _fuse_input(vertex_id, "vertex_id", torch.int32, n)
    if n > 0x7FFFFFFF:
        raise _lib.UcsaError("fuse_label_evidence: at most 2^31-1 pixels per call")
    if not (torch.is_tensor(scores) and scores.dim() >= 1
            and tuple(scores.shape) == tuple(vertex_id.shape) + (Cn,)):
        raise _lib.UcsaError(f"scores must be uint8 {list(vertex_id.shape) + [Cn]} (vertex_id's "
                             "shape, then the table's C)")
    sc = _fuse_input(scores, "scores", torch.uint8, n * Cn)
    if (mesh_depth is None) != (sensor_depth is None):
        raise _lib.UcsaError("mesh_depth and sensor_depth come as a pair")
    md = sd = None
    tol = 0.0
    if mesh_depth is not None:
        if depth_tol is None:
            raise _lib.UcsaError("the depth gate needs depth_tol")
        tol = float(depth_tol)
        if not tol >= 0.0:
            raise _lib.UcsaError(f"depth_tol must be >= 0, got {depth_tol}")
        md = _fuse_input(mesh_depth, "mesh_depth", torch.float32, n)
        sd = _fuse_input(sensor_depth, "sensor_depth", torch.float32, n)
    elif depth_tol is not None:
        raise _lib.UcsaError("depth_tol given without mesh_depth / sensor_depth")
    row_width = int(vertex_id.shape[-1]) if vertex_id.dim() >= 2 else 0
    check(lib().ucsa_label_fuse_evidence(
        _ptr(vid), _ptr(sc), _ptr(md), _ptr(sd), tol, n, row_width, V, Cn, _ptr(votes),
        votes.numel(), _stream()), "ucsa_label_fuse_evidence")
    return votes


# ---------------------------------------------------------------------------
# TSDF fusion (posed depth frames into a dense volume)
# ---------------------------------------------------------------------------
def tsdf_volume(dims, origin, spacing, with_color: bool = False, device="cuda"):
    """An empty TSDF volume for ``integrate_tsdf``: dict with ``tsdf`` [nx,ny,nz]
    f32 (ones: free), ``weight`` [nx,ny,nz] f32 (zeros: unobserved), ``rgb``
    [nx,ny,nz,3] f32 (zeros) or None, and the lattice ``origin`` / ``spacing``
    (3 floats each; point (i,j,k) at origin + (i,j,k)*spacing, poses' frame,
    scene units)."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7FFFFFFF:
        raise _lib.UcsaError(f"tsdf_volume: dims must be >= 2 each with at most 2^31-1 "
                             f"voxels, got {(nx, ny, nz)}")
    spacing = [float(spacing)] * 3 if isinstance(spacing, (int, float)) else \
        [float(v) for v in spacing]
    origin = [float(v) for v in origin]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("tsdf_volume: origin and spacing have 3 entries each")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.UcsaError("tsdf_volume: the volume lives on the GPU (no CPU fallback)")
    return {"tsdf": torch.ones(nx, ny, nz, device=dev),
            "weight": torch.zeros(nx, ny, nz, device=dev),
            "rgb": torch.zeros(nx, ny, nz, 3, device=dev) if with_color else None,
            "origin": tuple(origin), "spacing": tuple(spacing)}


def integrate_tsdf(volume, depth, poses, intrinsics, trunc: float, color=None,
                   max_weight: float = 65504.0, depth_min: float = 1e-6,
                   depth_max: float = 3.0e38):
    """Integrate B posed depth views into ``volume`` (``tsdf_volume``), in place;
    returns ``volume``.  ``depth`` [B,H,W] f32 z-depth in scene units (0, NaN,
    inf, anything outside [depth_min, depth_max] = no measurement), ``poses``
    [B,4,4] camera-to-world in the volume's frame, ``intrinsics`` (fx, fy, cx,
    cy) as for get_rays, ``trunc`` the truncation distance in scene units,
    ``color`` [B,H,W,3] uint8 iff the volume has ``rgb``.  Contract of
    ucsa_tsdf_integrate (include/ucsa_hip.h): a voxel's views are applied in
    order, so any split of the views over calls gives the same bytes."""
    for k in ("tsdf", "weight"):
        _inplace_f32(volume[k], f"volume['{k}']")
    tsdf, weight, rgb = volume["tsdf"], volume["weight"], volume.get("rgb")
    if tsdf.dim() != 3 or weight.shape != tsdf.shape or weight.device != tsdf.device:
        raise _lib.UcsaError("volume: tsdf and weight must be [nx,ny,nz] on one device")
    dev = tsdf.device
    if dev.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"the volume is on {dev} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    nx, ny, nz = (int(s) for s in tsdf.shape)
    if rgb is not None:
        _inplace_f32(rgb, "volume['rgb']")
        if rgb.shape != (nx, ny, nz, 3) or rgb.device != dev:
            raise _lib.UcsaError("volume: rgb must be [nx,ny,nz,3] on the volume's device")
    depth = _f32(depth, "depth")
    poses = _f32(poses, "poses")
    if depth.dim() != 3:
        raise _lib.UcsaError(f"depth must be [B,H,W], got {tuple(depth.shape)}")
    B, H, W = (int(s) for s in depth.shape)
    if poses.dim() != 3 or tuple(poses.shape) != (B, 4, 4):
        raise _lib.UcsaError(f"poses must be [{B},4,4], got {tuple(poses.shape)}")
    if depth.device != dev or poses.device != dev:
        raise _lib.UcsaError("depth and poses must be on the volume's device")
    if (color is None) != (rgb is None):
        raise _lib.UcsaError("color frames and a colour volume come as a pair")
    if color is not None:
        if not (torch.is_tensor(color) and color.is_cuda and color.device == dev):
            raise _lib.UcsaError("color must be a GPU tensor on the volume's device: the HIP "
                                 "path has no CPU fallback")
        if color.dtype != torch.uint8 or tuple(color.shape) != (B, H, W, 3):
            raise _lib.UcsaError(f"color must be uint8 [{B},{H},{W},3], got {color.dtype} "
                                 f"{tuple(color.shape)}")
        color = color.contiguous()
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    check(lib().ucsa_tsdf_integrate(
        _ptr(tsdf), _ptr(weight), _ptr(rgb), nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(color), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(max_weight), float(depth_min), float(depth_max),
        _stream()), "ucsa_tsdf_integrate")
    return volume


def tsdf_occupancy(volume, bound, cascade=None, H: int = 128, dilate=None,
                   min_weight: float = 1.0, free_tsdf: float = 1.0, unknown: str = "keep"):
    """Occupancy prior of a ``tsdf_volume`` for the marcher's cascade grid:
    uint8 [cascade,H,H,H] on the volume's device, 1 = the cell may hold matter,
    0 = every voxel its box meets was seen to be free space
    (``weight >= min_weight and tsdf >= free_tsdf``).  ``cascade`` None is the
    renderer's ``1 + ceil(log2(bound))``; ``dilate`` (scene units, grows every
    cell's box on all sides) None is the largest of the three spacings: one
    voxel, because the voxels that no view observed next to a surface hold no
    evidence either way; ``unknown`` "keep" keeps every cell that touches an
    unobserved voxel or reaches outside the volume, "empty" carves them.
    ``SemanticNeRFRenderer.set_occupancy_prior`` takes the result.  Contract of
    ucsa_tsdf_occupancy (include/ucsa_hip.h): a pure OR over a box of voxels,
    the same bytes every run."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    if unknown not in ("keep", "empty"):
        raise _lib.UcsaError(f"tsdf_occupancy: unknown must be 'keep' or 'empty', got {unknown!r}")
    bound = float(bound)
    if not (bound > 0 and math.isfinite(bound)):
        raise _lib.UcsaError(f"tsdf_occupancy: bound must be > 0 and finite, got {bound}")
    if cascade is None:
        cascade = 1 + math.ceil(math.log2(bound))
    cascade, H = int(cascade), int(H)
    if not 1 <= cascade <= 31:
        raise _lib.UcsaError(f"tsdf_occupancy: cascade must be in 1..31, got {cascade}")
    if not 2 <= H <= 1024:
        raise _lib.UcsaError(f"tsdf_occupancy: H must be in 2..1024, got {H}")
    spacing = [float(v) for v in volume["spacing"]]
    origin = [float(v) for v in volume["origin"]]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("tsdf_occupancy: origin and spacing have 3 entries each")
    if not all(v > 0 and math.isfinite(v) for v in spacing):
        raise _lib.UcsaError(f"tsdf_occupancy: spacing must be > 0 and finite, got {spacing}")
    if not all(math.isfinite(v) for v in origin):
        raise _lib.UcsaError(f"tsdf_occupancy: origin must be finite, got {origin}")
    dilate = max(spacing) if dilate is None else float(dilate)
    if not (dilate >= 0 and math.isfinite(dilate)):
        raise _lib.UcsaError(f"tsdf_occupancy: dilate must be >= 0 and finite, got {dilate}")
    if math.isnan(float(min_weight)) or math.isnan(float(free_tsdf)):
        raise _lib.UcsaError("tsdf_occupancy: min_weight and free_tsdf must not be NaN")
    mask = torch.empty(cascade, H, H, H, dtype=torch.uint8, device=dev)
    ws_bytes = int(lib().ucsa_tsdf_occupancy_workspace_bytes(nx, ny, nz))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    check(lib().ucsa_tsdf_occupancy(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        float(min_weight), float(free_tsdf), 1 if unknown == "keep" else 0, bound, cascade, H,
        dilate, _ptr(mask), mask.numel(), _ptr(ws), ws_bytes, _stream()), "ucsa_tsdf_occupancy")
    return mask


# ---------------------------------------------------------------------------
# voxel map (per-voxel class votes, ray-caster over the TSDF volume)
# ---------------------------------------------------------------------------
def _volume_lattice(volume):
    """(nx, ny, nz), device of a ``tsdf_volume`` checked as ``integrate_tsdf`` does"""
    for k in ("tsdf", "weight"):
        _inplace_f32(volume[k], f"volume['{k}']")
    tsdf, weight = volume["tsdf"], volume["weight"]
    if tsdf.dim() != 3 or weight.shape != tsdf.shape or weight.device != tsdf.device:
        raise _lib.UcsaError("volume: tsdf and weight must be [nx,ny,nz] on one device")
    dev = tsdf.device
    if dev.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"the volume is on {dev} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    rgb = volume.get("rgb")
    if rgb is not None:
        _inplace_f32(rgb, "volume['rgb']")
        if tuple(rgb.shape) != tuple(tsdf.shape) + (3,) or rgb.device != dev:
            raise _lib.UcsaError("volume: rgb must be [nx,ny,nz,3] on the volume's device")
    return tuple(int(s) for s in tsdf.shape), dev


def _u8_on(t, name, shape, dev):
    if not (torch.is_tensor(t) and t.is_cuda and t.device == dev):
        raise _lib.UcsaError(f"{name} must be a GPU tensor on the volume's device: the HIP "
                             "path has no CPU fallback")
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise _lib.UcsaError(f"{name} must be uint8 {list(shape)}, got {t.dtype} "
                             f"{tuple(t.shape)}")
    return t.contiguous()


def voxel_votes(volume, n_classes: int):
    """The zeroed vote table of a ``tsdf_volume`` for ``vote_voxel_labels``:
    [C+1, nx, ny, nz] uint16, class-major (plane = class id, plane 0 unused),
    1 <= C <= 255."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    Cn = int(n_classes)
    if not 1 <= Cn <= 255:
        raise _lib.UcsaError(f"voxel_votes: n_classes must be in 1..255, got {n_classes}")
    if (Cn + 1) * nx * ny * nz > 1 << 40:
        raise _lib.UcsaError("voxel_votes: (C+1)*nx*ny*nz must be at most 2^40")
    return torch.zeros(Cn + 1, nx, ny, nz, dtype=torch.uint16, device=dev)


def _vote_planes(votes):
    if not (torch.is_tensor(votes) and votes.is_cuda and votes.dtype == torch.uint16
            and votes.is_contiguous()):
        raise _lib.UcsaError("votes must be a contiguous uint16 tensor on the GPU")
    if votes.dim() != 4 or not 2 <= votes.shape[0] <= 256:
        raise _lib.UcsaError(f"votes must be [C+1,nx,ny,nz] with 1 <= C <= 255, got "
                             f"{tuple(votes.shape)}")
    return int(votes.shape[0]) - 1


def vote_voxel_labels(votes, volume, depth, pred, poses, intrinsics, trunc: float,
                      depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """B posed views vote into ``votes`` (``voxel_votes``), in place; returns
    ``votes``.  ``depth`` [B,H,W] f32, ``poses`` [B,4,4], ``intrinsics`` as for
    ``integrate_tsdf``; ``pred`` [B,H,W] uint8 class ids.  A voxel votes for
    pred's class at the pixel it projects to iff the depth there puts it in the
    band |z - c_z| <= trunc and 1 <= pred <= C; counts saturate at 65535.
    Contract of ucsa_tsdf_vote (include/ucsa_hip.h): independent of the TSDF
    state, and the same bytes for every split and order of the views."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    Cn = _vote_planes(votes)
    if tuple(votes.shape[1:]) != (nx, ny, nz) or votes.device != dev:
        raise _lib.UcsaError(f"votes must be [C+1,{nx},{ny},{nz}] on the volume's device, got "
                             f"{tuple(votes.shape)} on {votes.device}")
    depth = _f32(depth, "depth")
    poses = _f32(poses, "poses")
    if depth.dim() != 3:
        raise _lib.UcsaError(f"depth must be [B,H,W], got {tuple(depth.shape)}")
    B, H, W = (int(s) for s in depth.shape)
    if poses.dim() != 3 or tuple(poses.shape) != (B, 4, 4):
        raise _lib.UcsaError(f"poses must be [{B},4,4], got {tuple(poses.shape)}")
    if depth.device != dev or poses.device != dev:
        raise _lib.UcsaError("depth and poses must be on the volume's device")
    pred = _u8_on(pred, "pred", (B, H, W), dev)
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    check(lib().ucsa_tsdf_vote(
        _ptr(votes), votes.numel(), Cn, nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(pred), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(depth_min), float(depth_max), _stream()), "ucsa_tsdf_vote")
    return votes


def resolve_voxel_labels(votes, min_votes: int = 1):
    """``votes`` [C+1,nx,ny,nz] -> dict of device tensors [nx,ny,nz]: ``label``
    uint8 (the class with the most votes, ties to the lower id, 0 where the
    voxel's total is below ``min_votes``), ``total`` and ``winner`` uint32
    (confidence = winner / total).  ucsa_voxel_label_resolve."""
    Cn = _vote_planes(votes)
    min_votes = int(min_votes)
    if not 1 <= min_votes < 1 << 32:
        raise _lib.UcsaError(f"min_votes must be in 1..2^32-1, got {min_votes}")
    shape, dev = tuple(votes.shape[1:]), votes.device
    n = int(votes[0].numel())
    out = {"label": torch.empty(shape, dtype=torch.uint8, device=dev),
           "total": torch.empty(shape, dtype=torch.uint32, device=dev),
           "winner": torch.empty(shape, dtype=torch.uint32, device=dev)}
    check(lib().ucsa_voxel_label_resolve(_ptr(votes), Cn, n, min_votes, _ptr(out["label"]),
                                         _ptr(out["total"]), _ptr(out["winner"]), n,
                                         _stream()), "ucsa_voxel_label_resolve")
    return out


def voxel_evidence(volume, n_classes: int):
    """The zeroed evidence table of a ``tsdf_volume`` for
    ``accumulate_voxel_evidence``: [C+1, nx, ny, nz] uint32, class-major; plane
    c (1..C) is the evidence sum of class c, plane 0 the number of (view,
    voxel) contributions.  Limits as for ``voxel_votes``."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    Cn = int(n_classes)
    if not 1 <= Cn <= 255:
        raise _lib.UcsaError(f"voxel_evidence: n_classes must be in 1..255, got {n_classes}")
    if (Cn + 1) * nx * ny * nz > 1 << 40:
        raise _lib.UcsaError("voxel_evidence: (C+1)*nx*ny*nz must be at most 2^40")
    return torch.zeros(Cn + 1, nx, ny, nz, dtype=torch.uint32, device=dev)


def _evidence_planes(evidence):
    if not (torch.is_tensor(evidence) and evidence.is_cuda and evidence.dtype == torch.uint32
            and evidence.is_contiguous()):
        raise _lib.UcsaError("evidence must be a contiguous uint32 tensor on the GPU")
    if evidence.dim() != 4 or not 2 <= evidence.shape[0] <= 256:
        raise _lib.UcsaError(f"evidence must be [C+1,nx,ny,nz] with 1 <= C <= 255, got "
                             f"{tuple(evidence.shape)}")
    return int(evidence.shape[0]) - 1


def accumulate_voxel_evidence(evidence, volume, depth, scores, poses, intrinsics, trunc: float,
                              depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """The soft form of ``vote_voxel_labels``: B posed views add evidence into
    ``evidence`` (``voxel_evidence``), in place; returns ``evidence``.
    ``depth`` [B,H,W] f32, ``poses`` [B,4,4], ``intrinsics`` as for
    ``integrate_tsdf``; ``scores`` [B,H,W,C] uint8 (``log_evidence``).  A voxel
    takes the row of the pixel it projects to under exactly the rule of
    ``vote_voxel_labels`` (the band |z - c_z| <= trunc) unless the row is all
    zero, adds it to its C planes and 1 to plane 0; all adds saturate at
    2^32-1.  A voxel that no view of the call reaches is neither read nor
    written.  Contract of ucsa_tsdf_evidence (include/ucsa_hip.h): independent
    of the TSDF state, and the same bytes for every split and order of the
    views."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    Cn = _evidence_planes(evidence)
    if tuple(evidence.shape[1:]) != (nx, ny, nz) or evidence.device != dev:
        raise _lib.UcsaError(f"evidence must be [C+1,{nx},{ny},{nz}] on the volume's device, "
                             f"got {tuple(evidence.shape)} on {evidence.device}")
    depth = _f32(depth, "depth")
    poses = _f32(poses, "poses")
    if depth.dim() != 3:
        raise _lib.UcsaError(f"depth must be [B,H,W], got {tuple(depth.shape)}")
    B, H, W = (int(s) for s in depth.shape)
    if poses.dim() != 3 or tuple(poses.shape) != (B, 4, 4):
        raise _lib.UcsaError(f"poses must be [{B},4,4], got {tuple(poses.shape)}")
    if depth.device != dev or poses.device != dev:
        raise _lib.UcsaError("depth and poses must be on the volume's device")
    scores = _u8_on(scores, "scores", (B, H, W, Cn), dev)
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    check(lib().ucsa_tsdf_evidence(
        _ptr(evidence), evidence.numel(), Cn, nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(scores), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(depth_min), float(depth_max), _stream()),
        "ucsa_tsdf_evidence")
    return evidence


def resolve_voxel_evidence(evidence, min_views: int = 1, min_margin: int = 0):
    """``evidence`` [C+1,nx,ny,nz] -> dict of device tensors [nx,ny,nz]:
    ``label`` uint8 (the class with the largest evidence sum, ties to the lower
    id, 0 where plane 0 < ``min_views`` or margin < ``min_margin``), ``views``
    (plane 0), ``best`` and ``margin`` uint32 (best minus the runner-up; for
    C = 1 it is best).  ``label`` feeds ``raycast_tsdf(voxel_labels=...)``.
    ucsa_voxel_evidence_resolve."""
    Cn = _evidence_planes(evidence)
    min_views, min_margin = int(min_views), int(min_margin)
    if not 1 <= min_views < 1 << 32:
        raise _lib.UcsaError(f"min_views must be in 1..2^32-1, got {min_views}")
    if not 0 <= min_margin < 1 << 32:
        raise _lib.UcsaError(f"min_margin must be in 0..2^32-1, got {min_margin}")
    shape, dev = tuple(evidence.shape[1:]), evidence.device
    n = int(evidence[0].numel())
    out = {"label": torch.empty(shape, dtype=torch.uint8, device=dev),
           "views": torch.empty(shape, dtype=torch.uint32, device=dev),
           "best": torch.empty(shape, dtype=torch.uint32, device=dev),
           "margin": torch.empty(shape, dtype=torch.uint32, device=dev)}
    check(lib().ucsa_voxel_evidence_resolve(
        _ptr(evidence), Cn, n, min_views, min_margin, _ptr(out["label"]), _ptr(out["views"]),
        _ptr(out["best"]), _ptr(out["margin"]), n, _stream()), "ucsa_voxel_evidence_resolve")
    return out


def raycast_tsdf(volume, poses, intrinsics, H: int, W: int, near: float, far: float,
                 step: Optional[float] = None, min_weight: float = 1.0, voxel_labels=None,
                 trunc: Optional[float] = None, _plain_march: bool = False):
    """The model view of a TSDF volume from B posed cameras -> dict of device
    tensors: ``depth`` [B,H,W] f32 (z-depth of the first surface along the
    pixel's ray, 0 = miss), ``voxel_id`` [B,H,W] int32 (linear index of the
    nearest lattice point, -1 = miss), ``normal`` [B,H,W,3] f32 (world frame,
    toward free space), ``rgb`` [B,H,W,3] f32 when the volume has colour,
    ``label`` [B,H,W] int32 when ``voxel_labels`` [nx,ny,nz] uint8 is given.
    ``trunc`` is the truncation distance the volume was integrated with
    (default: ``volume["trunc"]``, which utils/voxel_map.py records);
    ``step`` the march step in scene units (default trunc / 2, must stay below
    trunc); only cells whose eight corners have weight >= ``min_weight`` are
    seen (the masked mesh's cell rule).  Contract of ucsa_tsdf_raycast
    (include/ucsa_hip.h); ``_plain_march`` selects the march without
    empty-space skipping, which gives the same bytes."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    poses = _f32(poses, "poses")
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.device != dev:
        raise _lib.UcsaError(f"poses must be [B,4,4] on the volume's device, got "
                             f"{tuple(poses.shape)} on {poses.device}")
    B, H, W = int(poses.shape[0]), int(H), int(W)
    if B < 1 or H < 1 or W < 1:
        raise _lib.UcsaError("raycast_tsdf: B, H, W must be >= 1")
    if trunc is None:
        trunc = volume.get("trunc")
    if trunc is None:
        raise _lib.UcsaError("raycast_tsdf: pass trunc, the truncation distance the volume "
                             "was integrated with (or record it as volume['trunc'])")
    trunc = float(trunc)
    step = 0.5 * trunc if step is None else float(step)
    rgb = volume.get("rgb")
    labels = None if voxel_labels is None else _u8_on(voxel_labels, "voxel_labels",
                                                       (nx, ny, nz), dev)
    out = {"depth": torch.empty(B, H, W, device=dev),
           "voxel_id": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "normal": torch.empty(B, H, W, 3, device=dev)}
    if rgb is not None:
        out["rgb"] = torch.empty(B, H, W, 3, device=dev)
    if labels is not None:
        out["label"] = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    ws, ws_bytes = None, 0
    if not _plain_march:
        ws_bytes = int(lib().ucsa_tsdf_raycast_workspace_bytes(nx, ny, nz))
        ws = _scratch_named("raycast", ws_bytes, dev)
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    check(lib().ucsa_tsdf_raycast(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), _ptr(rgb), _ptr(labels), nx, ny, nz,
        fvec(volume["origin"]), fvec(volume["spacing"]), _ptr(poses), B, fx, fy, cx, cy, H, W,
        float(near), float(far), trunc, step, float(min_weight), _ptr(out["depth"]),
        _ptr(out["voxel_id"]), _ptr(out["normal"]), _ptr(out.get("rgb")),
        _ptr(out.get("label")), B * H * W, _ptr(ws), ws_bytes, 1 if _plain_march else 0,
        _stream()), "ucsa_tsdf_raycast")
    return out


# ---------------------------------------------------------------------------
# neighbourhood pooling of the fused label tables
# ---------------------------------------------------------------------------
def _centre(centre) -> int:
    if isinstance(centre, bool) or not isinstance(centre, int) or not 1 <= centre <= 255:
        raise _lib.UcsaError(f"centre must be an integer in 1..255, got {centre!r}")
    return centre


def smooth_voxel_table(table, volume, neighbourhood: int = 26, iterations: int = 1,
                       centre: int = 1, min_weight: float = 1.0):
    """Pool a voxel table over each voxel's observed neighbours -> a NEW table
    of the same dtype and shape; ``table`` is not modified.  ``table``
    [C+1,nx,ny,nz], contiguous, on the volume's device: uint32
    (``voxel_evidence``) or uint16 (``voxel_votes``).  With obs(v) =
    ``volume["weight"][v] >= min_weight`` (fp32, the ray-caster's cell rule), a
    voxel with obs(v) gets, in every plane p = 0..C,
    min(SAT, centre * table[p, v] + the sum of table[p, n]) over its 6 face
    neighbours or the 26 neighbours of the 3x3x3 cube (``neighbourhood``) that
    lie inside the lattice and have obs(n); a voxel without obs(v) keeps its
    column.  SAT is 2^32-1 / 65535.  ``iterations`` = k gives the bytes of k
    single calls.  Plane 0 of an evidence table becomes a pooled contribution
    count: ``resolve_voxel_evidence(min_views=...)`` then applies to that count,
    and ``min_margin`` / ``min_votes`` to pooled sums (up to centre + 26 times a
    single voxel's).  Contract of ucsa_voxel_table_smooth (include/ucsa_hip.h)."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    if not (torch.is_tensor(table) and table.is_cuda
            and table.dtype in (torch.uint32, torch.uint16) and table.is_contiguous()):
        raise _lib.UcsaError("table must be a contiguous uint32 or uint16 tensor on the GPU")
    if table.dim() != 4 or not 2 <= table.shape[0] <= 256:
        raise _lib.UcsaError(f"table must be [C+1,nx,ny,nz] with 1 <= C <= 255, got "
                             f"{tuple(table.shape)}")
    if tuple(table.shape[1:]) != (nx, ny, nz) or table.device != dev:
        raise _lib.UcsaError(f"table must be [C+1,{nx},{ny},{nz}] on the volume's device, got "
                             f"{tuple(table.shape)} on {table.device}")
    if neighbourhood not in (6, 26):
        raise _lib.UcsaError(f"neighbourhood must be 6 or 26, got {neighbourhood!r}")
    centre = _centre(centre)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
        raise _lib.UcsaError(f"iterations must be an integer >= 1, got {iterations!r}")
    Cn = int(table.shape[0]) - 1
    weight = volume["weight"]
    src, spare = table, None
    for _ in range(iterations):
        dst = torch.empty_like(table) if spare is None else spare
        check(lib().ucsa_voxel_table_smooth(
            _ptr(src), _ptr(dst), table.element_size(), Cn, nx, ny, nz, _ptr(weight),
            float(min_weight), int(neighbourhood), centre, _stream()), "ucsa_voxel_table_smooth")
        # ping-pong between two fresh buffers; the input is only ever read
        spare = src if src is not table else None
        src = dst
    return src


def mesh_adjacency(faces, n_vertices: int):
    """The vertex adjacency of a triangle mesh as compressed rows, for
    ``smooth_label_table``: ``faces`` [F,3] int32 on the GPU -> (``offsets``
    int32 [V+1], ``neighbours`` int32 [E]); the neighbours of vertex v are
    ``neighbours[offsets[v]:offsets[v+1]]``, ascending.  Every undirected edge
    is stored once per direction, a face listed twice adds nothing, a
    degenerate face contributes only its proper edges (no self edges).  Plain
    torch on the device (sort and unique: plumbing, not a kernel)."""
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int32
            and faces.dim() == 2 and faces.shape[1] == 3):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the GPU")
    V = int(n_vertices)
    if not 0 <= V <= 0x7FFFFFFF:
        raise _lib.UcsaError(f"n_vertices must be in 0..2^31-1, got {n_vertices}")
    f = faces.long()
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
        raise _lib.UcsaError(f"faces index vertices outside 0..{V - 1}")
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    key = torch.unique(torch.cat([a * V + b, b * V + a]))       # sorted: by vertex, then neighbour
    if key.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("mesh_adjacency: more than 2^31-1 directed edges")
    src = torch.div(key, max(V, 1), rounding_mode="floor")
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=faces.device)
    offsets[1:] = torch.cumsum(torch.bincount(src, minlength=V), 0)
    return offsets.to(torch.int32), (key - src * V).to(torch.int32)


def smooth_label_table(votes, adjacency, iterations: int = 1, centre: int = 1):
    """Pool a mesh table over each vertex's neighbours -> a NEW table; ``votes``
    [V, C+1] int64 (the bits of the uint64 table of ``fuse_label_votes`` /
    ``fuse_label_evidence``) is not modified.  ``adjacency`` is
    ``mesh_adjacency``'s pair.  out[v, :] = centre * votes[v, :] + the sum of
    votes[n, :] over the neighbours n of v, in all C+1 columns, modulo 2^64; a
    vertex without neighbours gets centre * votes[v].  ``iterations`` = k gives
    the bytes of k single calls.  ``resolve_label_votes`` reads the result as
    it is; ``min_votes`` then counts pooled units.  Contract of
    ucsa_label_table_smooth (include/ucsa_hip.h)."""
    V, Cn = _vote_table(votes)
    if votes.device.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"votes is on {votes.device} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    try:
        offsets, neighbours = adjacency
    except (TypeError, ValueError):
        raise _lib.UcsaError("adjacency must be the (offsets, neighbours) pair of mesh_adjacency")
    for t, name in ((offsets, "offsets"), (neighbours, "neighbours")):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == votes.device
                and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous()):
            raise _lib.UcsaError(f"adjacency: {name} must be a contiguous int32 vector on the "
                                 "table's device")
    if offsets.numel() != V + 1:
        raise _lib.UcsaError(f"adjacency: offsets has {offsets.numel()} entries, the table has "
                             f"{V} vertices")
    centre = _centre(centre)
    if isinstance(iterations, bool) or not isinstance(iterations, int) or iterations < 1:
        raise _lib.UcsaError(f"iterations must be an integer >= 1, got {iterations!r}")
    src, spare = votes, None
    for _ in range(iterations):
        dst = torch.empty_like(votes) if spare is None else spare
        check(lib().ucsa_label_table_smooth(
            _ptr(src), _ptr(dst), V, Cn, _ptr(offsets), _ptr(neighbours), neighbours.numel(),
            centre, _stream()), "ucsa_label_table_smooth")
        spare = src if src is not votes else None
        src = dst
    return src


# ---------------------------------------------------------------------------
# connected components (voxel mask, mesh graph, component sizes)
# ---------------------------------------------------------------------------
def _on_current_device(t, name):
    if t.device.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"{name} is on {t.device} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")


def voxel_components(mask, connectivity: int = 26):
    """Connected components of a voxel mask -> int32 [nx,ny,nz]: the smallest
    linear index ``(i*ny + j)*nz + k`` of the voxel's component where ``mask``
    is set, -1 elsewhere.  ``mask`` [nx,ny,nz] bool or uint8 (non-zero = set) on
    the GPU; it is not modified.  ``connectivity`` 6 (face neighbours) or 26
    (the 3x3x3 cube), the neighbourhoods of ``smooth_voxel_table``.  Contract of
    ucsa_voxel_components (include/ucsa_hip.h)."""
    if not (torch.is_tensor(mask) and mask.is_cuda and mask.dtype in (torch.bool, torch.uint8)):
        raise _lib.UcsaError("mask must be a bool or uint8 tensor on the GPU: the HIP path has "
                             "no CPU fallback")
    if mask.dim() != 3 or mask.numel() == 0 or mask.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError(f"mask must be [nx,ny,nz] with 1 to 2^31-1 voxels, got "
                             f"{tuple(mask.shape)}")
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise _lib.UcsaError(f"connectivity must be 6 or 26, got {connectivity!r}")
    _on_current_device(mask, "mask")
    m = mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    nx, ny, nz = (int(s) for s in m.shape)
    labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=m.device)
    check(lib().ucsa_voxel_components(_ptr(m), _ptr(labels), nx, ny, nz, int(connectivity),
                                      _stream()), "ucsa_voxel_components")
    return labels


def mesh_components(adjacency):
    """Connected components of a mesh's vertex graph -> int32 [V]: the smallest
    vertex index of each vertex's component (an isolated vertex gets its own).
    ``adjacency`` is ``mesh_adjacency``'s (offsets, neighbours) pair; it is not
    modified.  Contract of ucsa_graph_components (include/ucsa_hip.h)."""
    try:
        offsets, neighbours = adjacency
    except (TypeError, ValueError):
        raise _lib.UcsaError("adjacency must be the (offsets, neighbours) pair of mesh_adjacency")
    for t, name in ((offsets, "offsets"), (neighbours, "neighbours")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 1
                and t.is_contiguous() and t.device == offsets.device):
            raise _lib.UcsaError(f"adjacency: {name} must be a contiguous int32 vector on the "
                                 "GPU, both on one device")
    if offsets.numel() < 1:
        raise _lib.UcsaError("adjacency: offsets has V + 1 entries, got none")
    _on_current_device(offsets, "adjacency")
    V = offsets.numel() - 1
    labels = torch.empty(V, dtype=torch.int32, device=offsets.device)
    check(lib().ucsa_graph_components(_ptr(offsets), _ptr(neighbours), V, neighbours.numel(),
                                      _ptr(labels), _stream()), "ucsa_graph_components")
    return labels


def component_sizes(labels):
    """The size of each element's component -> int32 of ``labels``' shape:
    the number of elements that carry ``labels[x]``, 0 where ``labels[x]`` < 0.
    ``labels`` int32 on the GPU, any shape, as ``voxel_components`` /
    ``mesh_components`` give it (values below the number of elements); it is not
    modified.  Contract of ucsa_component_sizes (include/ucsa_hip.h)."""
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int32):
        raise _lib.UcsaError("labels must be an int32 tensor on the GPU: the HIP path has no "
                             "CPU fallback")
    if labels.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("labels must have at most 2^31-1 elements")
    _on_current_device(labels, "labels")
    lab = labels.contiguous()
    sizes = torch.empty_like(lab)
    scratch = torch.empty_like(lab)
    check(lib().ucsa_component_sizes(_ptr(lab), _ptr(sizes), _ptr(scratch), lab.numel(),
                                     _stream()), "ucsa_component_sizes")
    return sizes


# ---------------------------------------------------------------------------
# nearest point within a radius (cell grid)
# ---------------------------------------------------------------------------
POINT_GRID_MAX_CELLS = 1 << 24


def _points3(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.shape[1] == 3):
        raise _lib.UcsaError(f"{name} must be an [N,3] tensor on the GPU: the HIP path has no "
                             "CPU fallback")
    if t.shape[0] > 0x7FFFFFFF:
        raise _lib.UcsaError(f"{name} must have at most 2^31-1 rows")
    return _f32(t, name)


def _finite_box(pts, ok):
    """the bounding box of the rows of ``pts`` [N,3] that ``ok`` marks (the finite
    ones) -> (lo, hi), three Python floats each; zeros when there is none"""
    if pts.shape[0] and bool(ok.any()):
        good = pts[ok]
        return good.min(0).values.tolist(), good.max(0).values.tolist()
    return [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]


def _cell_sort(keys, ncells: int):
    """int32 cell ``keys`` -> (``order`` int64: by key, ties by position;
    ``offsets`` int32 [ncells+1]: where each cell starts in that order)"""
    order = torch.sort(keys, stable=True).indices
    offsets = torch.searchsorted(keys[order].contiguous(),
                                 torch.arange(ncells + 1, dtype=torch.int32, device=keys.device)
                                 ).to(torch.int32)
    return order, offsets


def _search_args(grid, maker: str, payload: str, count: str, cols: int, queries, max_dist,
                 sort_queries: bool):
    """What ``nearest_point`` and ``nearest_triangle`` do before their library
    call: the queries, the grid dict of ops.``maker`` (its ``payload`` float32
    [grid[``count``], ``cols``]) and ``max_dist`` checked, and the queries' cell
    order -> (q, payload, offsets, n, origin, cell, dims, q_order, nq, max_dist)
    as the library takes them."""
    q = _points3(queries, "queries")
    try:
        pay, offsets = grid[payload], grid["offsets"]
        origin, cell, dims, n = grid["origin"], float(grid["cell"]), grid["dims"], int(grid[count])
    except (TypeError, KeyError):
        raise _lib.UcsaError(f"grid must be the dict of ops.{maker}")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    if not (torch.is_tensor(pay) and pay.is_cuda and pay.dtype == torch.float32
            and pay.is_contiguous() and tuple(pay.shape) == (n, cols) and torch.is_tensor(offsets)
            and offsets.dtype == torch.int32 and offsets.is_contiguous()
            and offsets.device == pay.device and offsets.numel() == ncells + 1):
        raise _lib.UcsaError(f"grid: {payload} must be float32 [{count},{cols}] and offsets int32 "
                             "[cells+1], contiguous, on one GPU")
    if pay.device != q.device:
        raise _lib.UcsaError(f"the grid is on {pay.device}, the queries on {q.device}")
    max_dist = float(max_dist)
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise _lib.UcsaError(f"max_dist must be positive and finite, got {max_dist!r}")
    nq = int(q.shape[0])
    org, dm = fvec(origin), (C.c_uint32 * 3)(*[int(d) for d in dims])
    q_order = None
    if sort_queries and nq and n:
        keys = torch.empty(nq, dtype=torch.int32, device=q.device)
        check(lib().ucsa_point_cell_keys(_ptr(q), nq, org, cell, dm, 0, _ptr(keys), _stream()),
              "ucsa_point_cell_keys")
        q_order = torch.sort(keys, stable=True).indices.to(torch.int32)
    return q, pay, offsets, n, org, cell, dm, q_order, nq, max_dist


def _grid_shape(lo, hi, n, cell):
    """origin, cell and dims from the finite points' box: host arithmetic in
    float64 on float32 corners.  The choice changes time only, never a result."""
    ext = [float(b) - float(a) for a, b in zip(lo, hi)]
    big = max(ext)
    if cell is None:
        pad = [e + max(big, 1e-30) * 1e-3 for e in ext]
        cell = (pad[0] * pad[1] * pad[2] / max(n, 1)) ** (1.0 / 3.0)
    cell = float(cell)
    if not (cell > 0 and math.isfinite(cell)):
        raise _lib.UcsaError(f"cell must be positive and finite, got {cell!r}")
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    cell = f32(max(cell, big / 1024.0, 1e-30))
    # more than 64 cells per point buy nothing and cost an offset each
    cap = min(POINT_GRID_MAX_CELLS, max(4096, 64 * n))
    while True:
        dims = tuple(int(math.floor(e / cell)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cap:
            return cell, dims
        cell = f32(cell * 1.25)


def point_grid(points, cell=None):
    """A uniform cell grid over ``points`` [N,3] (float32 on the GPU) for
    ``nearest_point`` -> dict: ``origin`` (3 floats) and ``dims`` (3 ints) from
    the finite points' bounding box, ``cell``, ``offsets`` int32 [cells+1],
    ``order`` int32 [N] (the points by cell, ties by index; non-finite points
    last), ``sorted_points`` float32 [N,4] (x, y, z and the bits of the original
    index in w), ``n``.  The default cell is the cube root of the padded box's
    volume per point, at least 1/1024 of the largest extent, and raised until
    the grid has at most min(2^24, max(4096, 64 N)) cells; an explicit ``cell``
    is raised the same way.  The cell changes time only, never a result.  The
    keys are a kernel (ucsa_point_cell_keys), the sort is torch on the device."""
    pts = _points3(points, "points")
    n = int(pts.shape[0])
    dev = pts.device
    lo, hi = _finite_box(pts, torch.isfinite(pts).all(1))
    cell, dims = _grid_shape(lo, hi, n, cell)
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib().ucsa_point_cell_keys(_ptr(pts), n, fvec(lo), cell, (C.c_uint32 * 3)(*dims), 1,
                                     _ptr(keys), _stream()), "ucsa_point_cell_keys")
    order64, offsets = _cell_sort(keys, dims[0] * dims[1] * dims[2])
    order = order64.to(torch.int32)
    packed = torch.empty((n, 4), dtype=torch.int32, device=dev)
    packed[:, :3] = pts[order64].view(torch.int32)
    packed[:, 3] = order
    return {"origin": tuple(float(v) for v in lo), "cell": cell, "dims": dims,
            "offsets": offsets, "order": order, "sorted_points": packed.view(torch.float32),
            "n": n}


def nearest_point(grid, queries, max_dist: float, sort_queries: bool = True):
    """For each of ``queries`` [Q,3] (float32 on the GPU) the nearest point of
    ``grid`` (``point_grid``'s dict) within ``max_dist`` -> (``index`` int32 [Q],
    ``dist2`` float32 [Q]) on the device: the original index of the nearest
    point and the squared distance, -1 and +inf where no point lies within
    ``max_dist`` (inclusive).  Among equally near points the smallest index
    wins; a non-finite point or query matches nothing.  ``max_dist`` is required
    and finite: an unbounded search is not offered, and a query with nothing
    near walks every cell within ``max_dist``, so passing the scene's diagonal
    costs what a brute-force search costs for such queries.  ``sort_queries``
    hands the queries to the kernel in cell order, so that a wave's lanes walk
    the same cells; it changes time only.  Contract of ucsa_nearest_point
    (include/ucsa_hip.h)."""
    q, sp, offsets, n, org, cell, dm, q_order, nq, max_dist = _search_args(
        grid, "point_grid", "sorted_points", "n", 4, queries, max_dist, sort_queries)
    index = torch.empty(nq, dtype=torch.int32, device=q.device)
    dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    check(lib().ucsa_nearest_point(_ptr(sp) if n else None, _ptr(offsets) if n else None, n, org,
                                   cell, dm, _ptr(q), _ptr(q_order), nq, max_dist, _ptr(index),
                                   _ptr(dist2), _stream()), "ucsa_nearest_point")
    return index, dist2


TRIANGLE_GRID_MAX_PAIRS = 0x7FFFFFFF


def triangle_grid(verts, faces, cell=None):
    """A uniform cell grid over the faces of a triangle mesh (``verts`` [V,3]
    float32, ``faces`` [F,3] int32, on the GPU) for ``nearest_triangle`` -> dict:
    ``origin`` (3 floats) and ``dims`` (3 ints) from the finite vertices'
    bounding box, ``cell``, ``offsets`` int32 [cells+1], ``records`` float32
    [P,12] (per (cell, face) pair, by cell and faces ascending inside a cell:
    A.xyz and the bits of the face index, B.xyz and 0, C.xyz and 0),
    ``n_pairs`` = P, ``n_faces``.  A face is registered in every cell of the box
    between its corners' cells; a face with a corner index outside [0, V) or a
    non-finite corner is registered nowhere.  The default cell is the (lower)
    median over the valid faces of the longest side of the face's box, at least
    1/1024 of the largest extent; it is raised by a quarter while the grid has
    more than min(2^24, max(4096, 64 F)) cells or more than max(65536, 32 F)
    pairs, and an explicit ``cell`` is raised the same way.  The cell changes
    time only, never a result.  Counts and pairs are kernels
    (ucsa_triangle_cell_counts, ucsa_triangle_cell_pairs); scan, sort and
    packing are torch on the device."""
    v = _points3(verts, "verts")
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dim() == 2 and faces.shape[1] == 3
            and faces.dtype == torch.int32 and faces.device == v.device):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the GPU of verts: the HIP "
                             "path has no CPU fallback")
    f = faces.contiguous()
    nv, nf = int(v.shape[0]), int(f.shape[0])
    if nf > 0x7FFFFFFF:
        raise _lib.UcsaError("faces must have at most 2^31-1 rows")
    if cell is not None and not (float(cell) > 0 and math.isfinite(float(cell))):
        raise _lib.UcsaError(f"cell must be positive and finite, got {cell!r}")
    dev = v.device
    fin = torch.isfinite(v).all(1)
    lo, hi = _finite_box(v, fin)
    ext = [float(b) - float(a) for a, b in zip(lo, hi)]
    big = max(ext)
    if cell is None:
        ok = ((f >= 0) & (f < nv)).all(1) if nv else torch.zeros(nf, dtype=torch.bool, device=dev)
        if nv and nf:
            ok &= fin[f.clamp(0, nv - 1).long()].all(1)
        if nf and bool(ok.any()):
            corners = v[f[ok].long()]                                   # [F',3,3]
            side = (corners.max(1).values - corners.min(1).values).max(1).values
            cell = float(torch.sort(side).values[(side.numel() - 1) // 2])
        else:
            cell = big
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    cell = f32(max(float(cell), big / 1024.0, 1e-30))
    cell_cap = min(POINT_GRID_MAX_CELLS, max(4096, 64 * nf))
    pair_cap = max(65536, 32 * nf)
    org = fvec(lo)
    counts = torch.empty(nf, dtype=torch.int32, device=dev)
    while True:
        dims = tuple(int(math.floor(e / cell)) + 1 for e in ext)
        if dims[0] * dims[1] * dims[2] <= cell_cap:
            dm = (C.c_uint32 * 3)(*dims)
            check(lib().ucsa_triangle_cell_counts(_ptr(v), nv, _ptr(f), nf, org, cell, dm,
                                                  _ptr(counts), _stream()),
                  "ucsa_triangle_cell_counts")
            n_pairs = int(counts.sum(dtype=torch.int64)) if nf else 0
            if n_pairs <= pair_cap:
                break
        cell = f32(cell * 1.25)
    if n_pairs > TRIANGLE_GRID_MAX_PAIRS:
        raise _lib.UcsaError(f"{n_pairs} (cell, face) pairs: at most 2^31-1")
    first = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).to(torch.int32)
    keys = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    pair_face = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    check(lib().ucsa_triangle_cell_pairs(_ptr(v), nv, _ptr(f), nf, org, cell, dm, _ptr(first),
                                         n_pairs, _ptr(keys), _ptr(pair_face), _stream()),
          "ucsa_triangle_cell_pairs")
    order, offsets = _cell_sort(keys, dims[0] * dims[1] * dims[2])
    sf = pair_face[order]
    rec = torch.zeros((n_pairs, 12), dtype=torch.int32, device=dev)
    if n_pairs:
        tri = f[sf.long()].long()
        for c in range(3):
            rec[:, 4 * c:4 * c + 3] = v[tri[:, c]].view(torch.int32)
        rec[:, 3] = sf
    return {"origin": tuple(float(x) for x in lo), "cell": cell, "dims": dims,
            "offsets": offsets, "records": rec.view(torch.float32), "n_pairs": n_pairs,
            "n_faces": nf}


def nearest_triangle(grid, queries, max_dist: float, sort_queries: bool = True):
    """For each of ``queries`` [Q,3] (float32 on the GPU) the nearest point on the
    faces of ``grid`` (``triangle_grid``'s dict) within ``max_dist`` -> (``face``
    int32 [Q], ``dist2`` float32 [Q], ``bary`` float32 [Q,3]) on the device: the
    face, the squared distance to its closest point and that point's
    barycentric weights of the face's three corners; -1, +inf and a zero row
    where no face lies within ``max_dist`` (inclusive).  Among equally near
    faces the smallest index wins; an invalid face or a non-finite query matches
    nothing.  ``max_dist`` is required and finite, as in ``nearest_point``, and
    costs the same: a query with nothing near walks every cell within it.
    ``sort_queries`` hands the queries to the kernel in cell order; it changes
    time only.  Contract of ucsa_nearest_triangle (include/ucsa_hip.h)."""
    q, rec, offsets, n, org, cell, dm, q_order, nq, max_dist = _search_args(
        grid, "triangle_grid", "records", "n_pairs", 12, queries, max_dist, sort_queries)
    face = torch.empty(nq, dtype=torch.int32, device=q.device)
    dist2 = torch.empty(nq, dtype=torch.float32, device=q.device)
    bary = torch.empty((nq, 3), dtype=torch.float32, device=q.device)
    check(lib().ucsa_nearest_triangle(_ptr(rec) if n else None, _ptr(offsets) if n else None, n,
                                      org, cell, dm, _ptr(q), _ptr(q_order), nq, max_dist,
                                      _ptr(face), _ptr(dist2), _ptr(bary), _stream()),
          "ucsa_nearest_triangle")
    return face, dist2, bary


# ---------------------------------------------------------------------------
# mesh simplification by vertex clustering
# ---------------------------------------------------------------------------
SIMPLIFY_MAX_DIM = 1 << 18
_NO_CLUSTER = 0x7FFFFFFFFFFFFFFF


def _vertex_rows(t, name, dtype, shape, dev):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.dtype == dtype
            and tuple(t.shape) == shape):
        raise _lib.UcsaError(f"{name} must be a {dtype} tensor of shape {list(shape)} on the "
                             "vertices' GPU")
    return t.contiguous()


def simplify_mesh(verts, faces, cell, normals=None, rgb=None, labels=None,
                  split_labels: bool = False, origin=None):
    """Simplify a triangle mesh by vertex clustering (Rossignac-Borrel): the
    vertices of one cell of a uniform grid of edge ``cell`` become one vertex.
    ``verts`` float32 [V,3] and ``faces`` int32 [F,3] on the GPU; per vertex and
    optional ``normals`` float32 [V,3], ``rgb`` uint8 [V,3], ``labels`` an
    integer tensor [V] with values 0..255 (0 = none).  A cluster is a cell; with
    ``split_labels`` it is a (cell, label) pair, so vertices of different
    classes in one cell are never merged and class borders keep their place.
    ``origin`` (3 floats) defaults to the minimum corner of the finite vertices;
    dims = floor(extent / cell) + 1 per axis, at most 2^18.  -> dict:
    ``verts`` float32 [K,3] (the members' mean, summed as offsets from the first
    member), ``count`` int32 [K] and, for the inputs given, ``normals`` (the
    normalised sum), ``rgb`` uint8 (the mean, half up), ``labels`` uint8 (the
    most frequent label > 0, ties to the smallest; 0 if none): one row per
    cluster, in ascending key order (x-major cell order, then label when
    split); ``faces`` int32 [F',3]: every face through the clusters of its
    corners, rotated to start at its smallest index, without the degenerate
    ones (two corners on one cluster, a corner outside [0, V) or on a
    non-finite vertex) and without repeated triples (the lowest input face is
    kept; a reversed copy is another triple and stays), in their former
    relative order; ``face_index`` int32 [F'] (the input face of each);
    ``vertex_map`` int32 [V] (the cluster of every input vertex, -1 for a
    non-finite one); ``origin``, ``cell``, ``dims``; ``degenerate`` and
    ``duplicate`` (how many faces went each way).  V = 0 and F = 0 are valid;
    the inputs are not modified.  One lane walks a cluster's members in order:
    a call that puts every vertex into one cell costs one lane walking all of
    them.  The keys, the per-cluster reduction and the face mapping are kernels
    (ucsa_vertex_cluster_keys, ucsa_cluster_reduce, ucsa_cluster_faces in
    include/ucsa_hip.h); the sort, the cluster boundaries, the de-duplication
    and the compaction are torch on the device."""
    pts = _points3(verts, "verts")
    dev = pts.device
    n = int(pts.shape[0])
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.device == dev
            and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the vertices' GPU")
    if faces.shape[0] > 0x7FFFFFFF:
        raise _lib.UcsaError("faces must have at most 2^31-1 rows")
    fc = faces.contiguous()
    nf = int(fc.shape[0])
    nrm = _vertex_rows(normals, "normals", torch.float32, (n, 3), dev)
    col = _vertex_rows(rgb, "rgb", torch.uint8, (n, 3), dev)
    lab = None
    if labels is not None:
        if not (torch.is_tensor(labels) and labels.is_cuda and labels.device == dev
                and not labels.dtype.is_floating_point and not labels.dtype.is_complex
                and labels.dtype != torch.bool and tuple(labels.shape) == (n,)):
            raise _lib.UcsaError(f"labels must be an integer tensor of shape [{n}] on the "
                                 "vertices' GPU")
        if n and (int(labels.min()) < 0 or int(labels.max()) > 255):
            raise _lib.UcsaError("labels must be in 0..255")
        lab = labels.to(torch.uint8).contiguous()
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    try:
        cell = f32(cell)
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"cell must be a number, got {cell!r}")
    if not (cell > 0 and math.isfinite(cell)):
        raise _lib.UcsaError(f"cell must be positive and finite in float32, got {cell!r}")
    lo, hi = _finite_box(pts, torch.isfinite(pts).all(1))
    if origin is not None:
        try:
            lo = [f32(v) for v in origin]
        except (TypeError, ValueError):
            raise _lib.UcsaError("origin must be three numbers")
        if len(lo) != 3 or not all(math.isfinite(v) for v in lo):
            raise _lib.UcsaError(f"origin must be three finite numbers, got {origin!r}")
    dims = tuple(int(math.floor(max(float(b) - float(a), 0.0) / cell)) + 1
                 for a, b in zip(lo, hi))
    if max(dims) > SIMPLIFY_MAX_DIM:
        raise _lib.UcsaError(f"cell {cell!r} needs {max(dims)} cells along an axis, more than "
                             f"2^18: raise cell")
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    check(lib().ucsa_vertex_cluster_keys(_ptr(pts), n, fvec(lo), cell, (C.c_uint32 * 3)(*dims),
                                         _ptr(lab), _ptr(keys), _stream()),
          "ucsa_vertex_cluster_keys")
    skeys, order64 = torch.sort(keys, stable=True)
    order = order64.to(torch.int32)
    n_fin = int((skeys != _NO_CLUSTER).sum()) if n else 0
    ident = skeys[:n_fin] if split_labels else skeys[:n_fin] >> 8
    _, inverse, counts = torch.unique_consecutive(ident, return_inverse=True, return_counts=True)
    K = int(counts.numel())
    first = torch.zeros(K + 1, dtype=torch.int32, device=dev)
    first[1:] = torch.cumsum(counts, 0)
    vertex_map = torch.full((n,), -1, dtype=torch.int32, device=dev)
    vertex_map[order64[:n_fin]] = inverse.to(torch.int32)
    out = {"verts": torch.empty((K, 3), dtype=torch.float32, device=dev),
           "count": torch.empty(K, dtype=torch.int32, device=dev)}
    if nrm is not None:
        out["normals"] = torch.empty((K, 3), dtype=torch.float32, device=dev)
    if col is not None:
        out["rgb"] = torch.empty((K, 3), dtype=torch.uint8, device=dev)
    if lab is not None:
        out["labels"] = torch.empty(K, dtype=torch.uint8, device=dev)
    check(lib().ucsa_cluster_reduce(_ptr(pts), _ptr(nrm), _ptr(col), _ptr(lab), n, _ptr(order),
                                    _ptr(first), K, _ptr(out["verts"]), _ptr(out.get("normals")),
                                    _ptr(out.get("rgb")), _ptr(out.get("labels")),
                                    _ptr(out["count"]), _stream()), "ucsa_cluster_reduce")
    tri = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    check(lib().ucsa_cluster_faces(_ptr(fc), nf, _ptr(vertex_map) if n else None, n, _ptr(tri),
                                   _ptr(keep), _stream()), "ucsa_cluster_faces")
    kept = torch.nonzero(keep).view(-1)
    n_kept = int(kept.numel())
    if n_kept:
        # equal triples, two columns at a time so that a key stays below 2^62
        t = tri[kept].long()
        ab = torch.unique(t[:, 0] * K + t[:, 1], return_inverse=True)[1]
        abc = torch.unique(ab * K + t[:, 2], return_inverse=True)[1]
        # a stable sort puts the lowest input face first in each group
        sg, pos = torch.sort(abc, stable=True)
        head = torch.ones_like(sg, dtype=torch.bool)
        head[1:] = sg[1:] != sg[:-1]
        face_index = kept[torch.sort(pos[head]).values]
    else:
        face_index = kept
    out["faces"] = tri[face_index].reshape(-1, 3)
    out["face_index"] = face_index.to(torch.int32)
    out["vertex_map"] = vertex_map
    out["origin"], out["cell"], out["dims"] = tuple(float(v) for v in lo), cell, dims
    out["degenerate"] = nf - n_kept
    out["duplicate"] = n_kept - int(face_index.numel())
    return out


# ---------------------------------------------------------------------------
# area-uniform sample points on a triangle mesh
# ---------------------------------------------------------------------------
SAMPLE_MAX_SAMPLES = 0x7FFFFFFF


def sample_mesh_surface(verts, faces, density, seed: int = 0, normals=None, rgb=None,
                        labels=None, max_samples: int = 1 << 26):
    """A deterministic, area-uniform, low-discrepancy point set on the surface of
    a triangle mesh, ``density`` points per unit area: the query points of 3D
    scores that weigh a surface by its area and not by its tessellation.
    ``verts`` float32 [V,3] and ``faces`` int32 [F,3] on the GPU; per vertex and
    optional ``normals`` float32 [V,3], ``rgb`` uint8 [V,3], ``labels`` an
    integer tensor [V] with values 0..255.  ``seed`` is a uint32.  -> dict:
    ``points`` float32 [S,3], ``face`` int32 [S] (ascending), ``bary`` float32
    [S,3] (multiples of 2^-24, non-negative, summing to exactly 1) and, for the
    inputs given, ``normals`` (the blend, normalised; zero where it vanishes),
    ``rgb`` uint8 (the blend, half up), ``labels`` uint8 (of the corner with the
    largest weight, the first on a tie, as ``transfer_labels`` decides); per
    face ``area`` float32 [F], ``count`` int32 [F] (area * density, rounded
    down after adding a hashed offset in [0, 1): no bias, so faces far smaller
    than 1 / density are sampled at the right rate) and ``first`` int32 [F+1]
    (the samples of face f are rows first[f] .. first[f+1]); ``n_samples`` = S
    and ``density`` (as rounded to float32).  A face with a corner index outside
    [0, V), a non-finite corner or a non-finite area has area 0 and no sample.
    A sample depends on (seed, face index, index inside the face) and the
    face's corners alone: a higher density keeps every earlier sample of a face
    and appends new ones, and editing one face moves no sample of another.
    More than ``max_samples`` (at most 2^31-1) samples is an error raised before
    anything of that size is allocated.  F = 0, V = 0 and S = 0 are valid; the
    inputs are not modified.  The counts and the samples are kernels
    (ucsa_face_sample_counts, ucsa_mesh_surface_samples in include/ucsa_hip.h);
    the prefix sum is torch on the device, in int64."""
    pts = _points3(verts, "verts")
    dev = pts.device
    n = int(pts.shape[0])
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.device == dev
            and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the vertices' GPU: the HIP "
                             "path has no CPU fallback")
    if faces.shape[0] > 0x7FFFFFFF:
        raise _lib.UcsaError("faces must have at most 2^31-1 rows")
    fc = faces.contiguous()
    nf = int(fc.shape[0])
    nrm = _vertex_rows(normals, "normals", torch.float32, (n, 3), dev)
    col = _vertex_rows(rgb, "rgb", torch.uint8, (n, 3), dev)
    lab = None
    if labels is not None:
        if not (torch.is_tensor(labels) and labels.is_cuda and labels.device == dev
                and not labels.dtype.is_floating_point and not labels.dtype.is_complex
                and labels.dtype != torch.bool and tuple(labels.shape) == (n,)):
            raise _lib.UcsaError(f"labels must be an integer tensor of shape [{n}] on the "
                                 "vertices' GPU")
        if n and (int(labels.min()) < 0 or int(labels.max()) > 255):
            raise _lib.UcsaError("labels must be in 0..255")
        lab = labels.to(torch.uint8).contiguous()
    try:
        density = float(torch.tensor(float(density), dtype=torch.float32))
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"density must be a number, got {density!r}")
    if not (density > 0 and math.isfinite(density)):
        raise _lib.UcsaError(f"density must be positive and finite in float32, got {density!r}")
    try:
        seed, max_samples = operator.index(seed), operator.index(max_samples)
    except TypeError:
        raise _lib.UcsaError("seed and max_samples must be integers")
    if not 0 <= seed <= 0xFFFFFFFF:
        raise _lib.UcsaError(f"seed must be in 0..2^32-1, got {seed!r}")
    if max_samples < 0:
        raise _lib.UcsaError(f"max_samples must not be negative, got {max_samples!r}")
    max_samples = min(max_samples, SAMPLE_MAX_SAMPLES)
    area = torch.empty(nf, dtype=torch.float32, device=dev)
    count = torch.empty(nf, dtype=torch.int32, device=dev)
    check(lib().ucsa_face_sample_counts(_ptr(pts) if n else None, n, _ptr(fc), nf, density, seed,
                                        _ptr(area), _ptr(count), _stream()),
          "ucsa_face_sample_counts")
    first64 = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    first64[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    S = int(first64[nf])
    if S > max_samples:
        raise _lib.UcsaError(f"density {density!r} gives {S} samples, more than max_samples = "
                             f"{max_samples}: lower density")
    first = first64.to(torch.int32)
    out = {"points": torch.empty((S, 3), dtype=torch.float32, device=dev),
           "face": torch.empty(S, dtype=torch.int32, device=dev),
           "bary": torch.empty((S, 3), dtype=torch.float32, device=dev)}
    if nrm is not None:
        out["normals"] = torch.empty((S, 3), dtype=torch.float32, device=dev)
    if col is not None:
        out["rgb"] = torch.empty((S, 3), dtype=torch.uint8, device=dev)
    if lab is not None:
        out["labels"] = torch.empty(S, dtype=torch.uint8, device=dev)
    check(lib().ucsa_mesh_surface_samples(_ptr(pts) if n else None, n, _ptr(fc), nf, _ptr(first), S,
                                          seed, _ptr(nrm), _ptr(col), _ptr(lab),
                                          _ptr(out["points"]), _ptr(out["face"]),
                                          _ptr(out["bary"]), _ptr(out.get("normals")),
                                          _ptr(out.get("rgb")), _ptr(out.get("labels")),
                                          _stream()), "ucsa_mesh_surface_samples")
    out.update(area=area, count=count, first=first, n_samples=S, density=density)
    return out


# ---------------------------------------------------------------------------
# mesh voxelization (the cells of a lattice or of the cascade grid a mesh meets)
# ---------------------------------------------------------------------------
VOXELIZE_LATTICE, VOXELIZE_CASCADE = 0, 1


def _voxelize(what, verts, faces, family, dims, origin, spacing, bound, cascade, dilate, out):
    pts = _points3(verts, "verts")
    dev = pts.device
    if dev.index != torch.cuda.current_device():
        raise _lib.UcsaError(f"the mesh is on {dev} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device first")
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.device == dev):
        raise _lib.UcsaError("faces must be a GPU tensor on the vertices' device: the HIP path "
                             "has no CPU fallback")
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise _lib.UcsaError(f"faces must be an integer tensor, got {faces.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise _lib.UcsaError(f"faces must be [F,3], got {tuple(faces.shape)}")
    V, F = int(pts.shape[0]), int(faces.shape[0])
    if F * cascade > 0x7FFFFFFF:
        raise _lib.UcsaError(f"{what}: faces x cascades must be at most 2^31-1")
    lo_hi = torch.stack(torch.aminmax(faces)).tolist() if F else [0, 0]
    if F and (lo_hi[0] < 0 or lo_hi[1] >= V):
        raise _lib.UcsaError(f"faces index outside [0, {V})")
    fc = _i32(faces.to(torch.int32).contiguous(), "faces")
    if not (dilate >= 0 and math.isfinite(dilate)):
        raise _lib.UcsaError(f"{what}: dilate must be >= 0 and finite, got {dilate}")
    nx, ny, nz = dims
    shape = (nx, ny, nz) if family == VOXELIZE_LATTICE else (cascade, nx, ny, nz)
    if out is None:
        mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        if not (torch.is_tensor(out) and out.is_cuda and out.device == dev
                and out.dtype == torch.uint8 and tuple(out.shape) == shape
                and out.is_contiguous()):
            raise _lib.UcsaError(f"out must be a contiguous uint8 {list(shape)} tensor on the "
                                 "vertices' device")
        mask = out
    o3 = fvec(origin) if origin is not None else None
    s3 = fvec(spacing) if spacing is not None else None
    geo = (_ptr(pts) if V else None, V, _ptr(fc) if F else None, F, family, nx, ny, nz, o3, s3,
           bound, cascade, dilate)
    items = F * cascade
    ws_bytes = int(lib().ucsa_mesh_voxelize_workspace_bytes(F, cascade))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev) if items else None
    count = torch.empty(items, dtype=torch.int32, device=dev) if items else None
    check(lib().ucsa_mesh_voxelize_count(*geo, _ptr(count), _ptr(ws), ws_bytes, _stream()),
          "ucsa_mesh_voxelize_count")
    first, total = None, 0
    if items:
        first = torch.zeros(items + 1, dtype=torch.int64, device=dev)
        first[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(first[items])
    check(lib().ucsa_mesh_voxelize_fill(*geo, _ptr(first), total, 0 if out is None else 1,
                                        _ptr(mask), mask.numel(), _ptr(ws), ws_bytes, _stream()),
          "ucsa_mesh_voxelize_fill")
    return mask


def voxelize_mesh(verts, faces, dims, origin, spacing, dilate: float = 0.0, out=None):
    """The voxels of a lattice that a triangle mesh passes through: uint8
    [nx,ny,nz] on the mesh's device, 1 = some face meets the voxel's box.  The
    lattice is ``tsdf_volume``'s: voxel (i,j,k) is the box of side ``spacing``
    (a number or 3) centred on origin + (i,j,k)*spacing, grown by ``dilate``
    (scene units) on every side; the mask can index a volume's arrays and go to
    ``voxel_components``.  ``verts`` float32 [V,3], ``faces`` an integer tensor
    [F,3] with indices in [0,V), both on the GPU; a face with a non-finite
    corner marks nothing, a segment or a point marks the voxels it touches.
    ``out`` (uint8 [nx,ny,nz], contiguous) accumulates: met voxels are set to 1
    and every other byte is left alone, so any split of the faces over calls
    gives the bytes of one call.  F = 0 gives an all-zero mask.  Contract of
    ucsa_mesh_voxelize_count / ucsa_mesh_voxelize_fill (include/ucsa_hip.h):
    conservative in float32 (a touching pair is never lost), a pure OR, the
    same bytes every run and for every face order.  Reads back the face index
    range (validation) and, between the two kernels, the column total."""
    try:
        dims = tuple(int(d) for d in dims)
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"voxelize_mesh: dims must be 3 integers, got {dims!r}")
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > 0x7FFFFFFF:
        raise _lib.UcsaError(f"voxelize_mesh: dims must be 3 integers >= 1 with at most 2^31-1 "
                             f"voxels, got {dims}")
    spacing = [float(spacing)] * 3 if isinstance(spacing, (int, float)) else \
        [float(v) for v in spacing]
    origin = [float(v) for v in origin]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("voxelize_mesh: origin and spacing have 3 entries each")
    if not all(v > 0 and math.isfinite(v) for v in spacing):
        raise _lib.UcsaError(f"voxelize_mesh: spacing must be > 0 and finite, got {spacing}")
    if not all(math.isfinite(v) for v in origin):
        raise _lib.UcsaError(f"voxelize_mesh: origin must be finite, got {origin}")
    return _voxelize("voxelize_mesh", verts, faces, VOXELIZE_LATTICE, dims, origin, spacing, 0.0,
                     1, float(dilate), out)


def mesh_occupancy(verts, faces, bound, cascade=None, H: int = 128, dilate=None, out=None):
    """Occupancy prior of a triangle mesh for the marcher's cascade grid: uint8
    [cascade,H,H,H] on the mesh's device, 1 = some face meets the cell's box, 0
    = the mesh does not come near the cell: a shell of cells around the
    surfaces.  ``SemanticNeRFRenderer.set_occupancy_prior`` takes the result.
    ``verts`` / ``faces`` as for ``voxelize_mesh``, in the field's (NGP) frame;
    ``bound`` the renderer's; ``cascade`` None is the renderer's
    ``1 + ceil(log2(bound))``, as in ``tsdf_occupancy``; ``dilate`` (scene
    units, grows every cell's box on all sides) None is one finest cell,
    ``2 * min(1, bound) / H``: a mesh is a surface estimate, and the field's
    surface may sit a cell beside it; ``out`` accumulates as in
    ``voxelize_mesh``.  F = 0 gives an all-zero mask.  Contract of
    ucsa_mesh_voxelize_count / ucsa_mesh_voxelize_fill (include/ucsa_hip.h)."""
    bound = float(bound)
    if not (bound > 0 and math.isfinite(bound)):
        raise _lib.UcsaError(f"mesh_occupancy: bound must be > 0 and finite, got {bound}")
    if cascade is None:
        cascade = 1 + math.ceil(math.log2(bound))
    cascade, H = int(cascade), int(H)
    if not 1 <= cascade <= 31:
        raise _lib.UcsaError(f"mesh_occupancy: cascade must be in 1..31, got {cascade}")
    if not 2 <= H <= 1024:
        raise _lib.UcsaError(f"mesh_occupancy: H must be in 2..1024, got {H}")
    dilate = 2.0 * min(1.0, bound) / H if dilate is None else float(dilate)
    return _voxelize("mesh_occupancy", verts, faces, VOXELIZE_CASCADE, (H, H, H), None, None,
                     bound, cascade, dilate, out)


# ---------------------------------------------------------------------------
# signed distance to a triangle mesh (pseudonormal sign, mesh to TSDF volume)
# ---------------------------------------------------------------------------
def _mesh_i32(verts, faces):
    v = _points3(verts, "verts")
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dim() == 2 and faces.shape[1] == 3
            and faces.dtype == torch.int32 and faces.device == v.device):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the GPU of verts: the HIP "
                             "path has no CPU fallback")
    if faces.shape[0] > 0x7FFFFFFF // 3:
        raise _lib.UcsaError("faces must have at most (2^31-1)/3 rows")
    return v, faces.contiguous()


def _normal_runs(items, run_first, n_runs, weight, unit, nf):
    out = torch.zeros((n_runs, 3), dtype=torch.float32, device=unit.device)
    check(lib().ucsa_normal_runs(_ptr(items) if items.numel() else None, _ptr(run_first), n_runs,
                                 int(items.numel()), _ptr(weight), _ptr(unit) if nf else None, nf,
                                 _ptr(out) if n_runs else None, _stream()), "ucsa_normal_runs")
    return out


def mesh_pseudonormals(verts, faces):
    """The normals the sign of ``signed_distance`` / ``mesh_tsdf`` is taken from
    (Baerentzen and Aanaes 2005) -> dict: ``unit_normal`` [F,3] (of
    (B-A)x(C-A); zeros for a degenerate or invalid face), ``corner_angle``
    [F,3] (radians, 0 for an invalid face), ``vertex_normal`` [V,3] (the sum
    over the faces at a vertex of corner angle * unit normal) and
    ``edge_normal`` [F,3,3] (row k of a face: the sum of the unit normals of all
    faces that share its edge corner k -> corner (k+1)%3), all float32 on the
    mesh's device, not normalised: only directions are used.  ``verts`` [V,3]
    float32, ``faces`` [F,3] int32, on the GPU; a face with a corner index
    outside [0,V) or a non-finite corner contributes nothing.  The unit normals
    and the two sums are kernels (ucsa_face_unit_normals, ucsa_normal_runs);
    the corner angles -- atan2(|u x w|, u.w) of the two edges leaving the corner
    -- and the stable sorts that group corners by vertex and half-edges by
    undirected edge are torch on the device.  The sorts are stable, so the
    items of a run ascend in 3f+k and every sum has one order."""
    v, f = _mesh_i32(verts, faces)
    dev = v.device
    nv, nf = int(v.shape[0]), int(f.shape[0])
    unit = torch.zeros((nf, 3), dtype=torch.float32, device=dev)
    check(lib().ucsa_face_unit_normals(_ptr(v) if nv else None, nv, _ptr(f) if nf else None, nf,
                                       _ptr(unit) if nf else None, _stream()),
          "ucsa_face_unit_normals")
    ok = ((f >= 0) & (f < nv)).all(1) if nv else torch.zeros(nf, dtype=torch.bool, device=dev)
    if nv and nf:
        ok &= torch.isfinite(v).all(1)[f.clamp(0, nv - 1).long()].all(1)
    angle = torch.zeros((nf, 3), dtype=torch.float32, device=dev)
    if nv and nf:
        P = v[f.clamp(0, nv - 1).long()]                                # [F,3 corners,3]
        for k in range(3):
            u, w = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            a = torch.atan2(torch.linalg.cross(u, w).norm(dim=1), (u * w).sum(1))
            angle[:, k] = torch.where(ok & torch.isfinite(a), a, torch.zeros_like(a))
    corner = torch.arange(3 * nf, dtype=torch.int32, device=dev)
    valid = ok.repeat_interleave(3)
    items0 = corner[valid]
    flat = f.reshape(-1).long()
    # vertices: the valid corners by vertex index, ties by 3f+k
    vid = flat[valid]
    order = torch.sort(vid, stable=True).indices
    v_items = items0[order].contiguous()
    v_first = torch.searchsorted(vid[order].contiguous(),
                                 torch.arange(nv + 1, dtype=torch.int64, device=dev)
                                 ).to(torch.int32)
    vertex_normal = _normal_runs(v_items, v_first, nv, angle.reshape(-1), unit, nf)
    # edges: the valid half-edges by undirected edge, ties by 3f+k
    nxt = f[:, [1, 2, 0]].reshape(-1).long()
    a, b = flat[valid], nxt[valid]
    key = torch.minimum(a, b) * max(nv, 1) + torch.maximum(a, b)
    order = torch.sort(key, stable=True).indices
    e_items = items0[order].contiguous()
    skey = key[order]
    n_half = int(skey.numel())
    head = torch.ones(n_half, dtype=torch.bool, device=dev)
    if n_half > 1:
        head[1:] = skey[1:] != skey[:-1]
    starts = torch.nonzero(head).reshape(-1)
    n_edges = int(starts.numel())
    e_first = torch.empty(n_edges + 1, dtype=torch.int32, device=dev)
    e_first[:n_edges] = starts
    e_first[n_edges] = n_half
    sums = _normal_runs(e_items, e_first, n_edges, None, unit, nf)
    edge_normal = torch.zeros((3 * nf, 3), dtype=torch.float32, device=dev)
    if n_half:
        edge_normal[e_items.long()] = sums[torch.cumsum(head, 0) - 1]
    return {"unit_normal": unit, "corner_angle": angle, "vertex_normal": vertex_normal,
            "edge_normal": edge_normal.view(nf, 3, 3)}


def _normals_args(normals, nv, nf, dev):
    try:
        un, vn, en = normals["unit_normal"], normals["vertex_normal"], normals["edge_normal"]
    except (TypeError, KeyError):
        raise _lib.UcsaError("normals must be the dict of ops.mesh_pseudonormals")
    for t, shape, name in ((un, (nf, 3), "unit_normal"), (vn, (nv, 3), "vertex_normal"),
                           (en, (nf, 3, 3), "edge_normal")):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev
                and tuple(t.shape) == shape and t.is_contiguous()):
            raise _lib.UcsaError(f"normals: {name} must be a contiguous float32 {list(shape)} "
                                 "tensor on the mesh's device (a different mesh?)")
    return (_ptr(un) if nf else None, _ptr(vn) if nv else None, _ptr(en) if nf else None)


def signed_distance(grid, normals, verts, faces, queries, max_dist: float,
                    sort_queries: bool = True):
    """For each of ``queries`` [Q,3] the signed distance to the mesh ``verts`` /
    ``faces`` within ``max_dist`` -> (``sdf`` float32 [Q], ``face``, ``dist2``,
    ``bary``, ``feature`` int32 [Q]): ``nearest_triangle`` (``grid`` is
    ``triangle_grid``'s dict of the same mesh; face, dist2 and bary are its
    outputs) followed by the sign.  ``abs(sdf)`` is ``sqrt(dist2)``; the sign is
    that of the angle-weighted pseudonormal (``normals``:
    ``mesh_pseudonormals``'s dict) of the feature the closest point lies on:
    ``feature`` 0 the face's interior, 1..3 its edges AB, BC, CA, 4..6 its
    corners A, B, C.  Positive is the side (B-A)x(C-A) points to: outside a
    mesh whose faces are counter-clockwise seen from outside.  No face within
    ``max_dist``: +inf and feature -1; a query on the surface: +0.  The sign is
    right wherever the mesh is a consistently oriented surface near the query;
    it is not a winding number and does not repair a badly oriented mesh.
    Contract of ucsa_mesh_sign (include/ucsa_hip.h)."""
    v, f = _mesh_i32(verts, faces)
    nv, nf = int(v.shape[0]), int(f.shape[0])
    try:
        grid_faces = int(grid["n_faces"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    if grid_faces != nf:
        raise _lib.UcsaError(f"grid was built over {grid_faces} faces, the mesh has {nf}")
    un, vn, en = _normals_args(normals, nv, nf, v.device)
    face, dist2, bary = nearest_triangle(grid, queries, max_dist, sort_queries)
    q = _points3(queries, "queries")
    if q.device != v.device:
        raise _lib.UcsaError(f"the mesh is on {v.device}, the queries on {q.device}")
    nq = int(q.shape[0])
    sdf = torch.empty(nq, dtype=torch.float32, device=q.device)
    feature = torch.empty(nq, dtype=torch.int32, device=q.device)
    check(lib().ucsa_mesh_sign(_ptr(v) if nv else None, nv, _ptr(f) if nf else None, nf, un, vn,
                               en, _ptr(q), nq, _ptr(face), _ptr(sdf), _ptr(feature), _stream()),
          "ucsa_mesh_sign")
    return sdf, face, dist2, bary, feature


def mesh_tsdf(volume, verts, faces, trunc: float, weight: float = 1.0, grid=None, normals=None):
    """Write the truncated signed distance to a mesh into ``volume``
    (``tsdf_volume``), in place; returns ``volume``.  Every voxel within
    ``trunc`` (scene units, inclusive) of the surface gets
    ``tsdf = clamp(sdf / trunc, -1, 1)`` and ``weight = weight``; every other
    voxel keeps what it held, so a fresh volume stays free and unobserved
    outside the band, as after ``integrate_tsdf``, and ``raycast_tsdf``,
    ``marching_cubes(valid=)``, ``tsdf_occupancy`` and ``voxel_components`` take
    the result.  The band is overwritten: the mesh is not averaged with what
    the volume held there, and ``rgb`` is not touched.  The sign is
    ``signed_distance``'s (positive on the side (B-A)x(C-A) points to, which is
    free space for a mesh that is counter-clockwise seen from outside).
    ``grid`` / ``normals`` are ``triangle_grid``'s and ``mesh_pseudonormals``'s
    dicts of the mesh, built here when not given.  One launch
    (ucsa_mesh_tsdf, include/ucsa_hip.h): the search runs from the lattice
    points themselves, byte for byte ``signed_distance`` on the materialised
    lattice."""
    (nx, ny, nz), dev = _volume_lattice(volume)
    v, f = _mesh_i32(verts, faces)
    if v.device != dev:
        raise _lib.UcsaError(f"the volume is on {dev}, the mesh on {v.device}")
    nv, nf = int(v.shape[0]), int(f.shape[0])
    trunc = float(trunc)
    if not (trunc > 0 and math.isfinite(trunc)):
        raise _lib.UcsaError(f"mesh_tsdf: trunc must be positive and finite, got {trunc!r}")
    weight = float(weight)
    if math.isnan(weight):
        raise _lib.UcsaError("mesh_tsdf: weight must not be NaN")
    origin = [float(x) for x in volume["origin"]]
    spacing = [float(x) for x in volume["spacing"]]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("mesh_tsdf: origin and spacing have 3 entries each")
    if grid is None:
        grid = triangle_grid(v, f)
    if normals is None:
        normals = mesh_pseudonormals(v, f)
    try:
        rec, offsets, n = grid["records"], grid["offsets"], int(grid["n_pairs"])
        g_origin, cell, dims, grid_faces = grid["origin"], float(grid["cell"]), grid["dims"], \
            int(grid["n_faces"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    if not (torch.is_tensor(rec) and rec.dtype == torch.float32 and rec.is_contiguous()
            and tuple(rec.shape) == (n, 12) and rec.device == dev and torch.is_tensor(offsets)
            and offsets.dtype == torch.int32 and offsets.is_contiguous()
            and offsets.device == dev and offsets.numel() == ncells + 1 and grid_faces == nf):
        raise _lib.UcsaError("grid: records must be float32 [n_pairs,12] and offsets int32 "
                             "[cells+1], contiguous, on the volume's GPU, built over this mesh")
    un, vn, en = _normals_args(normals, nv, nf, dev)
    check(lib().ucsa_mesh_tsdf(
        _ptr(rec) if n else None, _ptr(offsets) if n else None, n, fvec(g_origin), cell,
        (C.c_uint32 * 3)(*[int(d) for d in dims]), _ptr(v) if nv else None, nv,
        _ptr(f) if nf else None, nf, un, vn, en, _ptr(volume["tsdf"]), _ptr(volume["weight"]),
        nx, ny, nz, fvec(origin), fvec(spacing), trunc, weight, _stream()), "ucsa_mesh_tsdf")
    return volume
