"""Occupancy-grid ray marching: the marchers, their composites, ray compaction,
the density grid and the segmented marcher."""
from __future__ import annotations

import torch

from .._lib import check, lib
from ._args import _f32, _i32, _inplace_f32, _ptr, _scratch, _scratch_named, _stream


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
