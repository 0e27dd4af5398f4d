"""Inference: rays, sampling, the hash-grid encoders, the MLP packs and sigma
MLPs, resampling, compositing, point shading and the whole-view renders."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib
from .._lib import Grid, check, fvec, lib
from ._args import _f32, _ptr, _scratch_named, _stream


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
        raise _lib.UcsaError("hashgrid_encode_sorted: z_sorted / pix must hold N*T entries (pix uint8)")
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
        raise _lib.UcsaError("sigma_mlp_fwd_scatter: slot must be int32 [M]")
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


def _mlp_pack(symbol: str, kind: int, params, n_classes: int, out, size: str = "",
              per: int = 1, dtype=torch.float32, extra=()):
    """One launch of the library's pack ``symbol``.  ``out`` None: a new buffer of
    ``size``(kind, n_classes) // ``per`` elements of ``dtype`` (no ``size``: like
    ``params``).  ``extra``: arguments between n_classes and the stream."""
    params = _f32(params.detach(), "params")
    if out is None and not size:
        out = torch.empty_like(params)
    elif out is None:
        n = int(getattr(lib(), size)(kind, n_classes)) // per
        out = torch.empty(n, dtype=dtype, device=params.device)
    check(getattr(lib(), symbol)(kind, _ptr(params), _ptr(out), n_classes, *extra,
                                 _stream()), symbol)
    return out


def mlp_pack(kind: int, params: torch.Tensor, n_classes: int = 0,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _mlp_pack("ucsa_mlp_pack", kind, params, n_classes, out)


def _sigma_mlp_fwd(symbol: str, feat, packed_sigma):
    """feat [L,M,2] -> h [M,16], sigma [M] through the library's ``symbol``."""
    L, M, _ = feat.shape
    h = torch.empty(M, 16, device=feat.device)
    sigma = torch.empty(M, device=feat.device)
    check(getattr(lib(), symbol)(_ptr(feat), _ptr(packed_sigma), M, L, _ptr(h),
                                 _ptr(sigma), _stream()), symbol)
    return h, sigma


def sigma_mlp_fwd(feat, packed_sigma) -> Tuple[torch.Tensor, torch.Tensor]:
    """feat [L,M,2] -> h [M,16], sigma [M]."""
    return _sigma_mlp_fwd("ucsa_sigma_mlp_fwd", feat, packed_sigma)


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


def _composite_frame(rays_d, norms, z_c, z_f, n_classes: int):
    """What the composite forwards share: checked rays, the sizes and the three
    outputs -> (rays_d, norms, N, T, t, dev, image, depth, sem)."""
    rays_d = _f32(rays_d, "rays_d").view(-1, 3)
    norms = _f32(norms, "norms").view(-1)
    N, T = z_c.shape
    t = 0 if z_f is None else z_f.shape[1]
    dev = z_c.device
    return (rays_d, norms, N, T, t, dev, torch.empty(N, 3, device=dev),
            torch.empty(N, device=dev), torch.empty(N, n_classes, device=dev))


def composite_fwd(rays_d, norms, z_c, sigma_c, h_c, z_f, sigma_f, h_f,
                  packed_color, packed_sem, n_classes: int,
                  density_scale: float = 1.0, want_aux: bool = False,
                  half: bool = False):
    rays_d, norms, N, T, t, dev, image, depth, sem = _composite_frame(
        rays_d, norms, z_c, z_f, n_classes)
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
    rays_d, norms, N, T, t, dev, image, depth, sem = _composite_frame(
        rays_d, norms, z_c, z_f, n_classes)
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
    rays_d, norms, N, T, t, dev, image, depth, sem = _composite_frame(
        rays_d, norms, z_c, z_f, n_classes)
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


def _render_fwd(symbol: str, grid: Grid, table, packed_sigma, packed_color, packed_sem,
                rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t, n_classes,
                density_scale, image, depth, semantics, ws, image_width):
    """One chunk of run() through the library's ``symbol``; the packs are the
    ones that arithmetic reads."""
    N = rays_o.shape[0]
    check(getattr(lib(), symbol)(
        C.byref(grid), _ptr(table), _ptr(packed_sigma), _ptr(packed_color),
        _ptr(packed_sem), _ptr(rays_o), _ptr(rays_d), _ptr(norms), fvec(aabb),
        float(min_near), _ptr(t_rand), _ptr(u), N, T, t, n_classes,
        float(density_scale), int(image_width), _ptr(image), _ptr(depth),
        _ptr(semantics), _ptr(ws), _stream()), symbol)


def render_fwd(grid: Grid, table, packed_sigma, packed_color, packed_sem,
               rays_o, rays_d, norms, aabb, min_near: float, t_rand, u, T: int,
               t: int, n_classes: int, density_scale: float, image, depth,
               semantics, ws: torch.Tensor, image_width: int = 0):
    """All tensors already validated/contiguous; outputs written in place.
    image_width > 0: the rays are the pixels of full image rows."""
    _render_fwd("ucsa_render_fwd", grid, table, packed_sigma, packed_color, packed_sem,
                rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t, n_classes,
                density_scale, image, depth, semantics, ws, image_width)


# ======================= fp16-MFMA inference option =========================
def mlp_pack_f16(kind: int, params: torch.Tensor, n_classes: int = 0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    return _mlp_pack("ucsa_mlp_pack_f16", kind, params, n_classes, out,
                     "ucsa_mlp_pack_f16_halves", 1, torch.float16)


def mlp_pack_x3(kind: int, params: torch.Tensor, n_classes: int = 0,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weights as three bf16 terms per value in MFMA fragment order
    (csrc/mfma_mlp_x3.h)."""
    return _mlp_pack("ucsa_mlp_pack_x3", kind, params, n_classes, out,
                     "ucsa_mlp_pack_x3_bytes", 2, torch.bfloat16)


def mlp_pack_h2(kind: int, params: torch.Tensor, n_classes: int = 0,
                out: Optional[torch.Tensor] = None,
                range_bits: Optional[torch.Tensor] = None,
                scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weights as two f16 terms per value (the second scaled by 2^11) in MFMA
    fragment order (csrc/mfma_mlp_h2.h, "f16x2").  ``range_bits`` (int32 [1] in
    pinned host or device memory, zeroed by the caller) accumulates the largest
    |value| converted to f16 as an fp32 bit pattern; ``scratch``: int32 [2] on
    the device, zeroed once (ucsa_mlp_pack_h2_checked)."""
    size = ("ucsa_mlp_pack_h2_bytes", 2, torch.float16)
    if range_bits is None:
        return _mlp_pack("ucsa_mlp_pack_h2", kind, params, n_classes, out, *size)
    if scratch is None or not scratch.is_cuda or scratch.numel() < 2:
        raise _lib.UcsaError("mlp_pack_h2: range_bits needs a 2-word int32 device scratch")
    return _mlp_pack("ucsa_mlp_pack_h2_checked", kind, params, n_classes, out, *size,
                     extra=(_ptr(range_bits), _ptr(scratch)))


def sigma_mlp_fwd_h2(feat, packed_sigma_h2):
    return _sigma_mlp_fwd("ucsa_sigma_mlp_fwd_h2", feat, packed_sigma_h2)


def render_fwd_h2(grid: Grid, table, packed_sigma_h2, packed_color_h2,
                  packed_sem_h2, rays_o, rays_d, norms, aabb, min_near: float,
                  t_rand, u, T: int, t: int, n_classes: int,
                  density_scale: float, image, depth, semantics,
                  ws: torch.Tensor, image_width: int = 0):
    """run() with the three nets as f16x2 (fp32-grade on the f16 MFMA pipe,
    three passes per product)."""
    _render_fwd("ucsa_render_fwd_h2", grid, table, packed_sigma_h2, packed_color_h2,
                packed_sem_h2, rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t,
                n_classes, density_scale, image, depth, semantics, ws, image_width)


def sigma_mlp_fwd_f16(feat, packed_sigma_half):
    if feat.dtype == torch.float16:   # features of the fp16-table encoder
        return _sigma_mlp_fwd("ucsa_sigma_mlp_fwd_f16_h", feat, packed_sigma_half)
    return _sigma_mlp_fwd("ucsa_sigma_mlp_fwd_f16", feat, packed_sigma_half)


def render_fwd_f16(grid: Grid, table, packed_sigma_h, packed_color_h,
                   packed_sem_h, rays_o, rays_d, norms, aabb, min_near: float,
                   t_rand, u, T: int, t: int, n_classes: int,
                   density_scale: float, image, depth, semantics,
                   ws: torch.Tensor, image_width: int = 0):
    _render_fwd("ucsa_render_fwd_f16", grid, table, packed_sigma_h, packed_color_h,
                packed_sem_h, rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t,
                n_classes, density_scale, image, depth, semantics, ws, image_width)


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
    assert table_half.dtype == torch.float16
    _render_fwd("ucsa_render_fwd_f16_h16", grid, table_half, packed_sigma_h, packed_color_h,
                packed_sem_h, rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t,
                n_classes, density_scale, image, depth, semantics, ws, image_width)


def sigma_mlp_fwd_x3(feat, packed_sigma_x3):
    return _sigma_mlp_fwd("ucsa_sigma_mlp_fwd_x3", feat, packed_sigma_x3)


def render_fwd_x3(grid: Grid, table, packed_sigma_x3, packed_color_x3,
                  packed_sem_x3, rays_o, rays_d, norms, aabb, min_near: float,
                  t_rand, u, T: int, t: int, n_classes: int,
                  density_scale: float, image, depth, semantics,
                  ws: torch.Tensor, image_width: int = 0):
    """run() with the three nets as bf16x3 (fp32-grade on the bf16 MFMA pipe)."""
    _render_fwd("ucsa_render_fwd_x3", grid, table, packed_sigma_x3, packed_color_x3,
                packed_sem_x3, rays_o, rays_d, norms, aabb, min_near, t_rand, u, T, t,
                n_classes, density_scale, image, depth, semantics, ws, image_width)


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
