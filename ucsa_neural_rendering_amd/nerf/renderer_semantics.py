"""Mirror of reference ``nr4seg/nerf/renderer_semantics.py``.

Same class, constructor, buffers and ``run`` / ``render`` signatures
(reference :63-103, :123-135, :301-310).  ``run`` is one enqueue of the HIP
pipeline (``ucsa_render_fwd``) instead of ~80 torch ops and three tcnn calls.

Extra OPTIONAL keyword arguments: ``num_steps``,
``upsample_steps`` (already accepted through ``**kwargs`` by the reference),
``rng_t`` [N,T] and ``rng_u`` [N,t] to supply the uniforms the reference draws
with ``torch.rand`` (:166 and sample_pdf :28) so results can be compared
value-for-value.
"""
from __future__ import annotations

import math
import os
from typing import NamedTuple

import numpy as np

import torch
import torch.nn as nn

from .. import ops


class Arithmetic(NamedTuple):
    """What a ``precision`` selects.  The ops are NAMES, looked up in ``ops`` at
    the call, so that replacing ``ops.NAME`` (lab tools, tests) still takes."""
    form: str           # pack form of the three nets (SemanticNeRFNetwork._nets)
    half_table: bool    # read the hash grid from the fp16 copy of the table
    sigma_mlp: str      # ops.sigma_mlp_fwd*
    render: str         # ops.render_fwd*: one chunk of run()
    view: str           # mode of ops.render_view: all chunks as one call


# keyed by ``precision``; ``fp16_table`` selects "fp16_h16" (see __init__ for what
# each arithmetic is)
PRECISIONS = {
    "fp32": Arithmetic("f32", False, "sigma_mlp_fwd", "render_fwd", "fp32"),
    "fp16": Arithmetic("h", False, "sigma_mlp_fwd_f16", "render_fwd_f16", "fp16"),
    "fp16_h16": Arithmetic("h", True, "sigma_mlp_fwd_f16", "render_fwd_f16_h16", "fp16_h16"),
    "bf16x3": Arithmetic("x3", False, "sigma_mlp_fwd_x3", "render_fwd_x3", "bf16x3"),
    "f16x2": Arithmetic("h2", False, "sigma_mlp_fwd_h2", "render_fwd_h2", "f16x2"),
}


class SemanticNeRFRenderer(nn.Module):

    def __init__(self, bound=1, cuda_ray=False, density_scale=1,
                 num_semantic_classes=41):
        super().__init__()
        self.epoch = 1
        self.weights = np.zeros([0])
        self.weights_sum = np.zeros([0])
        self.bound = bound
        self.cascade = 1 + math.ceil(math.log2(bound))
        self.density_scale = density_scale
        self.num_semantic_classes = num_semantic_classes
        aabb_train = torch.FloatTensor(
            [-bound, -bound, -bound, bound, bound, bound])
        aabb_infer = aabb_train.clone()
        self.register_buffer("aabb_train", aabb_train)
        self.register_buffer("aabb_infer", aabb_infer)
        # extra state for occupancy-grid marching (reference :89-103)
        self.cuda_ray = cuda_ray
        if cuda_ray:
            density_grid = torch.zeros([self.cascade] + [128] * 3)
            self.register_buffer("density_grid", density_grid)
            self.mean_density = 0
            self.iter_density = 0
            step_counter = torch.zeros(16, 2, dtype=torch.int32)
            self.register_buffer("step_counter", step_counter)
            self.mean_count = 0
            self.local_step = 0
        # cuda_ray=True: render() marches for inference; training goes through
        # run() (the reference's behaviour) unless march_training is set
        self.march_training = False
        # rays per HIP enqueue; results do not depend on it
        self.hip_ray_chunk = 65536
        # chunks are independent and may alternate over several HIP streams;
        # measured on MI355X: no gain (every kernel already fills the chip),
        # so one stream by default
        self.hip_streams = 1
        # no-grad renders of >= 2 chunks as one software-pipelined call
        # (ucsa_render_view: density half of chunk k+1 || shading half of chunk k)
        self.hip_pipeline = os.environ.get("UCSA_RENDER_PIPELINE", "1") != "0"
        # the pipelined call balances its chunks: ceil(N / min(hip_ray_chunk, this)) of them
        self.hip_pipeline_rays = int(os.environ.get("UCSA_PIPELINE_RAYS", "65536"))
        # inference (no-grad render) arithmetic of the three MLPs:
        #   "fp32"   f32-input MFMA, bit for bit a k-ordered fmaf chain (the
        #            same kernels arithmetic as the training forward);
        #   "bf16x3" fp32-grade on the bf16 MFMA pipe: every operand split
        #            exactly into three bf16 terms, six partial products per
        #            product, fp32 accumulation (csrc/mfma_mlp_x3.h) -- within
        #            1-2 ulp of "fp32", ~25 % less time per view;
        #   "f16x2"  fp32-grade on the f16 MFMA pipe with HALF the matrix passes
        #            of bf16x3: every operand as two f16 terms (the second
        #            scaled by 2^11), three partial products per product
        #            (csrc/mfma_mlp_h2.h); layer inputs and weights must stay
        #            below 65504 (the range of the reference's own fp16 nets), hidden activations
        #            below 2^20; out-of-range values are not detected;
        #   "fp16"   what tiny-cuda-nn does (fp16 weights and layer inputs,
        #            fp32 accumulation).
        self.precision = "fp32"
        # with precision="fp16": also read the hash grid from an fp16 copy of
        # the table, as tiny-cuda-nn stores it (fp32 master with the
        # optimizer); off by default -- the fp16 mode's parity fixtures are
        # stated for the fp32 table
        self.fp16_table = False
        # training through run(): "fp32" (default, the parity path) or "fp16":
        # colour / semantics nets forward AND backward on f16 MFMA (fp16
        # weights / layer inputs / incoming gradients, fp32 accumulation, fp32
        # weight gradients); sigma net and hash grid stay fp32.  f16_bwd_scale
        # is tiny-cuda-nn's loss scale for the f16 gradient operands (set it to
        # 1 when the incoming gradients already carry a GradScaler scale).
        self.train_precision = "fp32"
        # with train_precision="bf16x3": the backward's contractions of the
        # colour / semantics nets -- "bf16x2" (default: bf16 MFMA pipe, two-term
        # operand splits, 2^-16 per product; gradients within the 2e-3 of the
        # oracle the fp32 kernels are held to) or "fp32" (f32-input MFMA)
        self.bwd_precision = "bf16x2"
        # hash-grid backward of a training step: both density passes in ONE call
        # that walks every ray's samples in sorted depth order
        # (ucsa_hashgrid_bwd_rays_merged) instead of one call per pass
        self.grid_bwd_merged = os.environ.get("UCSA_GRID_BWD_MERGED", "1") != "0"
        # with the bf16x2 backward: the hash-grid backward's bin records are
        # 8-byte words with 26-bit values (ucsa_hashgrid_bwd_rays*_p64) instead
        # of 16-byte (index, fp32, fp32) records -- half the record traffic
        self.grid_records_packed = os.environ.get("UCSA_GRID_RECORDS_PACKED", "1") != "0"
        # the default training mode (bf16x3 / bf16x2 / packed / merged) as ONE C
        # call per direction (ucsa_render_fused_fwd / ucsa_render_fused_bwd)
        # instead of one call per stage from Python; bit-identical
        self.fused_train_calls = os.environ.get("UCSA_FUSED_TRAIN", "1") != "0"
        # with train_precision="bf16x3": the FORWARD nets of the training pass as
        # f16x2 (two-term f16 operands, three MFMA passes per product instead of
        # six, the same fp32-grade error; csrc/mfma_mlp_h2.h) -- the backward
        # keeps its bf16 packs
        self.train_fwd_f16x2 = os.environ.get("UCSA_TRAIN_FWD_F16X2", "1") != "0"
        self.f16_bwd_scale = 1024.0
        # with train_precision="fp16": the hash-grid backward's bin records
        # carry half2 values (8 instead of 16 bytes per record)
        self.f16_grid_records = True
        self._side_streams = []
        self._ws = None
        self._aabb_host = {}

    def forward(self, x, d):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def reset_extra_state(self):
        """reference :111-121."""
        if not self.cuda_ray:
            return
        self.density_grid.zero_()
        if getattr(self, "occupancy_prior", None) is not None:
            self.density_grid[self.occupancy_prior == 0] = -1.0
        self.mean_density = 0
        self.iter_density = 0
        self.step_counter.zero_()
        self.mean_count = 0
        self.local_step = 0

    # -- occupancy prior: measured free space, carved for good ----------------
    # ucsa_density_grid_update leaves a negative cell alone and counts it as 0 in
    # the mean, and the marcher's grid > thresh never enters one: a cell set to
    # -1 here stays empty whatever the field says there.  ops.tsdf_occupancy /
    # utils/occupancy_prior.py make the mask from the scene's depth frames.
    @torch.no_grad()
    def set_occupancy_prior(self, mask):
        """``mask`` [cascade,H,H,H] (uint8 / bool, 1 = may hold matter) in
        density_grid's layout: every 0 cell becomes -1 in density_grid, for
        good (update_extra_state never touches it, the marcher never samples
        it); a 1 cell that was negative (an earlier prior) goes back to 0 and is
        learned from the field as usual.  The mask is kept as a non-persistent
        buffer (it follows ``.to()``, the state_dict keys do not change) and
        reset_extra_state re-applies it.  mean_density stays the mean over ALL
        cells with the carved ones counted as 0, as in the parent code base:
        under a tight prior it is smaller, so the marcher's threshold
        min(0.01, mean_density) can only become more permissive."""
        if not self.cuda_ray:
            raise ValueError("set_occupancy_prior needs cuda_ray=True: only the marcher "
                             "reads density_grid")
        mask = torch.as_tensor(mask)
        if tuple(mask.shape) != tuple(self.density_grid.shape):
            raise ValueError(f"occupancy prior must be {tuple(self.density_grid.shape)} like "
                             f"density_grid, got {tuple(mask.shape)}")
        mask = (mask != 0).to(device=self.density_grid.device, dtype=torch.uint8).contiguous()
        if "occupancy_prior" in self._buffers:
            self.occupancy_prior = mask
        else:
            self.register_buffer("occupancy_prior", mask, persistent=False)
        keep = mask != 0
        self.density_grid[~keep] = -1.0
        self.density_grid[keep & (self.density_grid < 0)] = 0.0

    @torch.no_grad()
    def clear_occupancy_prior(self):
        """Drop the prior: the carved cells go back to 0 and the next refreshes
        learn them from the field."""
        if "occupancy_prior" in self._buffers:
            del self._buffers["occupancy_prior"]
            self._non_persistent_buffers_set.discard("occupancy_prior")
        if self.cuda_ray:
            self.density_grid[self.density_grid < 0] = 0.0

    # -- occupancy-grid marching ---------------------------
    # The reference keeps the state above and the raymarching functions but no
    # code that drives them (its parent code base had `update_extra_state` and
    # `run_cuda`; this fork dropped both and hard-codes cuda_ray=False).  The
    # two methods below are that driver, written for this build.
    @torch.no_grad()
    def update_extra_state(self, decay=None, seed=None):
        """Refresh density_grid from the field: one jittered sample per cell
        and cascade, grid = max(grid*decay, density_scale*sigma); then
        mean_density, and mean_count from the step counters of the last
        training steps.  Call before rendering and every 16 training steps.

        ``decay`` defaults to 0.6 for the first 16 refreshes and 0.95 after:
        a freshly initialised field has sigma ~ 1 everywhere, and with 0.95
        alone the grid needs ~90 refreshes to fall below the marcher's fixed
        0.01 threshold (measured: 413 points per ray for the first 1400
        training steps, 40 afterwards)."""
        if not self.cuda_ray:
            return
        if decay is None:
            decay = 0.6 if self.iter_density < 16 else 0.95
        H = self.density_grid.shape[1]
        dev = self.density_grid.device
        if seed is None:
            seed = self.iter_density + 1
        fresh = torch.empty_like(self.density_grid)
        for cas in range(self.cascade):
            pts = ops.density_grid_points(cas, H, float(self.bound), int(seed),
                                          dev)
            fresh[cas] = self.density(pts)["sigma"].view(H, H, H)
        mean = ops.density_grid_update(self.density_grid, fresh, float(decay),
                                       float(self.density_scale))
        self.iter_density += 1
        total_step = min(16, self.local_step)
        # one read-back for both numbers (each one drains the queue)
        points = self.step_counter[:max(total_step, 1), 0].sum()
        mean_v, points_v = torch.stack(
            [mean.view(()).double(), points.double()]).tolist()
        self.mean_density = float(mean_v)
        if total_step > 0:
            self.mean_count = int(points_v / total_step)
        self.local_step = 0

    @staticmethod
    def refresh_due(step: int) -> bool:
        """When a training loop should call ``update_extra_state``: every 16
        steps, and every 8 during the first 128.  A fresh field has sigma ~ 1
        everywhere and the grid forgets it by 0.6 per refresh, so the air is
        marched densely (~700 points per ray, ~10 ms per step) until the
        ninth refresh; refreshing twice as often there empties it by step
        ~100 instead of ~150-200 (measured: 3.1 -> 2.65 ms per step averaged
        over the first 600 steps, same PSNR / mIoU; every 4 steps gains
        nothing more, a refresh costs 3.7 ms)."""
        return step % 16 == 0 or (step < 128 and step % 8 == 0)

    def _march_render_fn(self):
        raise NotImplementedError

    def _run_cuda_train(self, rays_o, rays_d, direction_norms, dt_gamma=0,
                        perturb=False, min_near=0.2, w_min=1e-4,
                        force_all_rays=False, **kwargs):
        """Differentiable marched pass (what the reference's parent code did in
        training with cuda_ray=True): march_rays_train with the running
        mean_count as the point budget (the first 16 steps, or
        force_all_rays, read the exact count back), then the fused field +
        composite.  Depth follows ``run``: sum w*t / |d|; there is no far
        closure here -- a field trained this way carries its own opacity."""
        from .raymarching import raymarching
        prefix = rays_o.shape[:-1]
        device = rays_o.device
        if device.type != "cuda":
            raise ops._lib.UcsaError(
                "run_cuda needs GPU tensors: the HIP path has no CPU fallback")
        o = rays_o.contiguous().view(-1, 3).float()
        d = rays_d.contiguous().view(-1, 3).float()
        nrm = direction_norms.contiguous().view(-1).float()
        C = self.num_semantic_classes
        N = o.shape[0]
        if N == 0:
            return {
                "depth": torch.empty(*prefix, device=device),
                "image": torch.empty(*prefix, 3, device=device),
                "semantics": torch.empty(*prefix, C, device=device),
                "weights_sum": torch.empty(*prefix, device=device),
            }
        aabb = self._aabb_list(self.training)
        with torch.no_grad():
            nears, fars = ops.near_far_from_aabb(o, d, aabb, min_near)
            counter = self.step_counter[self.local_step % 16]
            counter.zero_()
            self.local_step += 1
            # budget = 1.05 x the running mean.  The per-step total of 4096 rays
            # varies by ~1.5 %: with the bare mean about every second step
            # overflows and drops its last rays (reference
            # raymarching.py:111-116 accepts that).  The slack is not free --
            # the field kernels run on all `budget` rows, zero-filled or not --
            # hence 5 %, not more (1.25 x measured: 3.0 -> 4.1 ms per step).
            budget = int(self.mean_count * 1.05) if self.mean_count > 0 else -1
            xyzs, _, deltas, rays = raymarching.march_rays_train(
                o, d, self.bound, self.density_grid, self.mean_density, nears,
                fars, counter, budget, perturb, 128, force_all_rays, dt_gamma)
        image, depth, sem, ws = self._march_render_fn()(
            self, o, d, nrm, nears, xyzs, deltas, rays, float(w_min))
        return {
            "depth": depth.view(*prefix),
            "image": image.view(*prefix, 3),
            "semantics": sem.view(*prefix, C),
            "weights_sum": ws.view(*prefix),
        }

    def run_cuda(self, rays_o, rays_d, direction_norms, **kwargs):
        """Render by occupancy-grid marching: the differentiable training pass
        (_run_cuda_train) when gradients are enabled and parameters require
        them, else the inference loop (_run_cuda_infer)."""
        if torch.is_grad_enabled() and any(p.requires_grad
                                           for p in self.parameters()):
            keep = {k: kwargs[k] for k in ("dt_gamma", "perturb", "min_near",
                                           "w_min", "force_all_rays")
                    if k in kwargs}
            return self._run_cuda_train(rays_o, rays_d, direction_norms, **keep)
        kwargs.pop("force_all_rays", None)
        return self._run_cuda_infer(rays_o, rays_d, direction_norms, **kwargs)

    @torch.no_grad()
    def _run_cuda_infer(self, rays_o, rays_d, direction_norms, dt_gamma=0,
                 bg_color=None, perturb=False, max_steps=1024, epoch=None,
                 min_near=0.2, far_closure=True, schedule="segments",
                 march_caps=(32, 96, 1024), w_min=1e-4, fused_shade=True,
                 **kwargs):
        """Inference by occupancy-grid marching with early termination and
        alive-ray compaction (march_rays -> field -> composite_rays ->
        compact_rays until no ray is alive).  Same inputs / outputs and the
        same depth convention as ``run`` (depth = sum w*t / |d|).

        ``far_closure``: ``run`` makes the last interval of every ray 1e10
        wide (reference :185-186, :238-239), i.e. the sample at ``far`` absorbs
        whatever transmittance is left, and fields trained through ``run``
        rely on it.  With far_closure=True the marcher ends every ray the same
        way (one extra sample at t = far with delta 1e10), so it renders the
        same model as ``run`` and can be swapped in for it; False gives the
        plain marching integral.

        ``schedule``: "segments" (default) marches in a few rounds of up to
        ``march_caps`` samples per alive ray with exact-size buffers and the
        alive count kept on the device; "reference" is the loop the reference
        API was made for (n_step <= 8 samples per iteration, zero-padded
        buffers, one host sync per iteration).  Both take the same samples.

        ``fused_shade`` (segments only): form the weights first and run the
        colour / semantics nets only on the samples with w > ``w_min``, inside
        one kernel (ucsa_march_segment_shade).  w_min = 1e-4 is the mask of
        ``run`` (reference :249-250); 0 shades every sample like the
        reference's composite_rays.  ``self.precision = "fp16"`` selects the
        fp16-MFMA nets here as it does in ``run``."""
        from .raymarching import raymarching
        prefix = rays_o.shape[:-1]
        device = rays_o.device
        if device.type != "cuda":
            raise ops._lib.UcsaError(
                "run_cuda needs GPU tensors: the HIP path has no CPU fallback")
        o = rays_o.contiguous().view(-1, 3).float()
        d = rays_d.contiguous().view(-1, 3).float()
        nrm = direction_norms.contiguous().view(-1).float()
        N = o.shape[0]
        C = self.num_semantic_classes
        if N == 0:
            return {
                "depth": torch.empty(*prefix, device=device),
                "image": torch.empty(*prefix, 3, device=device),
                "semantics": torch.empty(*prefix, C, device=device),
                "weights_sum": torch.empty(*prefix, device=device),
            }
        aabb = self._aabb_list(self.training)
        nears, fars = ops.near_far_from_aabb(o, d, aabb, min_near)
        f, sigma_mlp, shade_mode, shade_nets = self._march_arith(
            schedule == "segments" and fused_shade)
        ws = torch.zeros(N, device=device)
        depth = torch.zeros(N, device=device)
        image = torch.zeros(N, 3, device=device)
        sem = torch.zeros(N, C, device=device)
        self.last_march_points = 0
        self.last_march_rounds = 0
        if schedule == "segments":
            # MI355X-native driver: a few rounds of exact-size spans, the alive
            # count stays on the device, one host read-back per round
            seg = ops.MarchSegments(o, d, nears, fars, self.density_grid,
                                    self.mean_density, self.bound, dt_gamma)
            n_cap, done = N, 0
            for cap in march_caps:
                cap = min(int(cap), max_steps - done)
                if cap <= 0 or n_cap == 0:
                    break
                jitter = int(perturb) if done == 0 else 0
                total, n_alive = seg.count(n_cap, cap, jitter)
                if n_alive == 0:
                    break
                if total > 0:
                    xyzs, dirs, deltas = seg.write(n_alive, total, jitter)
                    feat = ops.hashgrid_encode_points(f["grid"], f["table"],
                                                      xyzs)
                    h, sigma = sigma_mlp(feat)
                    if fused_shade:
                        seg.shade(n_alive, cap, sigma,
                                  float(self.density_scale), h, deltas,
                                  shade_nets["packed_color"], shade_nets["packed_sem"], C,
                                  float(w_min), ws, depth, image, sem, shade_mode)
                    else:
                        rgbs, probs = ops.point_shade_h(
                            dirs, h, f["packed_color"], f["packed_sem"], C)
                        seg.composite(n_alive, cap, sigma,
                                      float(self.density_scale), rgbs, probs,
                                      deltas, ws, depth, image, sem)
                    seg.compact(n_alive)
                self.last_march_points += total
                self.last_march_rounds += 1
                n_cap = n_alive if total > 0 else 0
                done += cap
            rays_alive, rays_t = seg.alive, seg.t
        elif schedule == "reference":
            # the loop of the reference API, one host sync per iteration
            rays_alive = torch.empty(2, N, dtype=torch.int32, device=device)
            rays_alive[0] = torch.arange(N, dtype=torch.int32, device=device)
            rays_t = torch.empty(2, N, device=device)
            rays_t[0] = nears
            alive_counter = torch.zeros(1, dtype=torch.int32, device=device)
            n_alive, step, i = N, 0, 0
            while step < max_steps and n_alive > 0:
                a, b = i % 2, (i + 1) % 2
                n_step = max(min(N // n_alive, 8), 1)
                xyzs, dirs, deltas = raymarching.march_rays(
                    n_alive, n_step, rays_alive[a], rays_t[a], o, d,
                    self.bound, self.density_grid, self.mean_density, nears,
                    fars, 128, int(perturb), dt_gamma)
                feat = ops.hashgrid_encode_points(f["grid"], f["table"], xyzs)
                h, sigma = ops.sigma_mlp_fwd(feat, f["packed_sigma"])
                if self.density_scale != 1:
                    sigma = sigma * self.density_scale
                rgbs, probs = ops.point_shade_h(dirs, h, f["packed_color"],
                                                f["packed_sem"], C)
                raymarching.composite_rays_semantics(
                    n_alive, n_step, rays_alive[a], rays_t[a], sigma, rgbs,
                    probs, deltas, ws, depth, image, sem)
                alive_counter.zero_()
                raymarching.compact_rays(n_alive, rays_alive[b], rays_alive[a],
                                         rays_t[b], rays_t[a], alive_counter)
                self.last_march_points += n_alive * n_step
                self.last_march_rounds += 1
                n_alive = int(alive_counter.item())
                step += n_step
                i += 1
        else:
            raise ValueError(f"unknown schedule {schedule!r}")
        if far_closure:
            f = self._field()
            feat = ops.hashgrid_encode_rays(f["grid"], f["table"], o, d,
                                            fars.view(N, 1), aabb)
            h, sigma = ops.sigma_mlp_fwd(feat, f["packed_sigma"])
            rgbs, probs = ops.point_shade_h(d, h, f["packed_color"],
                                            f["packed_sem"], C)
            last = torch.zeros(N, 2, device=device)
            last[:, 0] = 1e10
            rays_alive[0] = torch.arange(N, dtype=torch.int32, device=device)
            rays_t[0] = fars
            raymarching.composite_rays_semantics(
                N, 1, rays_alive[0], rays_t[0], sigma, rgbs, probs, last, ws,
                depth, image, sem)
        return {
            "depth": (depth / nrm).view(*prefix),
            "image": image.view(*prefix, 3),
            "semantics": sem.view(*prefix, C),
            "weights_sum": ws.view(*prefix),
        }

    # -- hooks supplied by the field (SemanticNeRFNetwork) -------------------
    def _field(self):
        raise NotImplementedError()

    def _nets(self, form: str, transposed: bool = False):
        raise NotImplementedError()

    def _table_half(self):
        raise NotImplementedError()

    def _arithmetic(self, fp16_table=None) -> Arithmetic:
        """The row of PRECISIONS that ``precision`` and ``fp16_table`` select."""
        if self.precision not in ("fp32", "fp16", "bf16x3", "f16x2"):
            raise ValueError("precision must be fp32, bf16x3, f16x2 or fp16, got "
                             f"{self.precision}")
        half_table = self.fp16_table if fp16_table is None else fp16_table
        if half_table and self.precision != "fp16":
            raise ValueError("fp16_table needs precision='fp16' (its encoder emits "
                             "fp16 features, which only the f16 sigma MLP reads)")
        return PRECISIONS["fp16_h16" if half_table else self.precision]

    def _march_arith(self, fused: bool):
        """The marcher's arithmetic -> (field ``f``, sigma MLP of the marched points
        as a callable of the features, ``shade_mode`` and nets of the fused shading
        kernel).  That kernel has f32-input, f16 and -- round 6 -- f16x2 nets: with
        bf16x3 the colour / semantics nets shade in fp32 here; the sigma MLP of the
        marched points runs on the 16-bit pipe in the selected arithmetic -- round
        6: it used to fall back to the f32-input MFMA, 0.33 instead of 0.21 ms per
        5.9 M points.  fp16 nets run only with the fused kernel, everything else is
        fp32 then.  The marcher always reads the fp32 table."""
        row = self._arithmetic(fp16_table=False)
        if self.precision == "fp16" and not fused:
            row = PRECISIONS["fp32"]
        half = row.form == "h"
        f = self._nets("h") if half else self._field()
        sigma_nets = f if row.form in ("h", "f32") else self._nets(row.form)
        shade_mode, shade_nets = half, f
        if row.form == "h2" and fused:
            shade_mode, shade_nets = "f16x2", sigma_nets

        def sigma_mlp(feat):
            return getattr(ops, row.sigma_mlp)(feat, sigma_nets["packed_sigma"])
        return f, sigma_mlp, shade_mode, shade_nets

    def _aabb_list(self, training: bool):
        key = bool(training)
        buf = self.aabb_train if training else self.aabb_infer
        ver = buf._version
        hit = self._aabb_host.get(key)
        if hit is None or hit[0] != ver:
            self._aabb_host[key] = (ver, [float(v) for v in buf.detach().cpu()])
        return self._aabb_host[key][1]

    def _workspace(self, nbytes: int, device, slots: int = 1):
        # one workspace per (device, caller stream): two streams rendering with
        # one module at the same time must not share the intermediates
        # ucsa_render_view / ucsa_render_fwd* write; at most four are
        # kept (a module is normally driven from one or two streams)
        if self._ws is None:
            self._ws = {}
        key = (str(device), int(torch.cuda.current_stream(device).cuda_stream))
        ws = self._ws.get(key)
        if ws is None or ws.shape[0] < slots or ws.shape[1] < nbytes:
            if ws is None and len(self._ws) >= 4:
                self._ws.pop(next(iter(self._ws)))
            ws = torch.empty(slots, nbytes, dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def run(self, rays_o, rays_d, direction_norms, num_steps=256,
            upsample_steps=256, bg_color=None, perturb=False, epoch=None,
            rng_t=None, rng_u=None, min_near=0.2, image_width=0, **kwargs):
        """reference :123-299.  rays [B,N,3], direction_norms [B,N,1] ->
        {"depth" [B,N], "image" [B,N,3], "semantics" [B,N,C]}.
        ``bg_color`` is accepted and unused, exactly like the reference
        (:288-289 assigns it, nothing reads it).

        ``image_width`` (optional, inference): set it when the N rays are the
        pixels of full rows of an image that wide (what ``get_rays`` returns):
        the hash-grid gather then walks 8x8 pixel tiles, whose lanes share
        cells (ucsa_hashgrid_encode_rays_image).  Same results."""
        prefix = rays_o.shape[:-1]
        device = rays_o.device
        if device.type != "cuda":
            raise ops._lib.UcsaError(
                "SemanticNeRFRenderer.run needs GPU tensors: the HIP path has "
                "no CPU fallback")
        o = rays_o.contiguous().view(-1, 3).float()
        d = rays_d.contiguous().view(-1, 3).float()
        nrm = direction_norms.contiguous().view(-1).float()
        N = o.shape[0]
        T, t = int(num_steps), int(upsample_steps)
        C = self.num_semantic_classes
        if perturb and rng_t is None:
            rng_t = torch.rand(N, T, device=device)
        if not perturb:
            rng_t = None
        if t > 0 and rng_u is None:
            rng_u = torch.rand(N, t, device=device)
        if rng_t is not None:
            rng_t = rng_t.reshape(N, T).float().contiguous()
        if rng_u is not None:
            rng_u = rng_u.reshape(N, t).float().contiguous()
        aabb = self._aabb_list(self.training)

        if N == 0:
            return {
                "depth": torch.empty(*prefix, device=device),
                "image": torch.empty(*prefix, 3, device=device),
                "semantics": torch.empty(*prefix, C, device=device),
            }
        if torch.is_grad_enabled() and any(
                p.requires_grad for p in self.parameters()):
            out = self._run_train(o, d, nrm, aabb, T, t, rng_t, rng_u, min_near)
        else:
            out = self._run_infer(o, d, nrm, aabb, T, t, rng_t, rng_u, min_near,
                                  int(image_width))
        image, depth, sem = out
        return {
            "depth": depth.view(*prefix),
            "image": image.view(*prefix, 3),
            "semantics": sem.view(*prefix, C),
        }

    def infer_chunk(self, N: int, image_width: int = 0, samples_per_ray: int = 0):
        """(rays per enqueue, image_width or 0) of a no-grad render of N rays:
        ``hip_ray_chunk`` at most; whole 8-row bands of 8x8 pixel tiles when the
        rays are full image rows; and, for the pipelined call, >= 2 BALANCED
        chunks (a 320x240 frame is 2 x 38 400 rays, not 65 536 + 11 264).
        Measured on the 640x480 view (tools/chunk_sweep.py): 15.7 - 16.1 M
        rays/s for any chunk between 20 k and 150 k rays, one 307 k chunk 15.3;
        the joint step: 192 ms unpipelined, 187 / 184 ms with 2 / 3 chunks per
        frame.  Larger launches keep the encoder's per-launch efficiency (the
        bench's roofline figure), hence hip_ray_chunk as the cap.  The pipelined
        call's budget is in SAMPLES beyond 192 per ray (~10 M per chunk): the
        joint step's 8 frames of 320x240 at 256 + 256 samples go out as 30
        chunks of 20 480 rays instead of 10 of 61 440 (round 4, with the faster
        f16x2 shader: 167 -> 163 ms).
        Results do not depend on any of it."""
        chunk = max(1, int(self.hip_ray_chunk))
        band = 8 * image_width if (image_width and N % image_width == 0) else 0
        if self.hip_pipeline and int(self.hip_streams) <= 1 and N > 16384:
            budget = max(64, self.hip_pipeline_rays)
            if samples_per_ray > 192:   # ~10 M samples per chunk
                budget = max(8192, budget * 192 * 4 // (samples_per_ray * 5))
            n = max(2, -(-N // min(chunk, budget)))
            chunk = -(-N // n)
            unit = band if band and chunk >= band else 64
            chunk = -(-chunk // unit) * unit
        if band and chunk >= band:
            chunk -= chunk % band  # whole 8-row bands of tiles
        else:
            image_width = 0
        return chunk, image_width

    def _run_infer(self, o, d, nrm, aabb, T, t, rng_t, rng_u, min_near,
                   image_width=0):
        row = self._arithmetic()
        f = self._nets(row.form)
        if row.half_table:
            f["table"] = self._table_half()
        if row.form == "h2" and self._h2_guard_mode() == "full":
            self._h2_check_activations(o, d, aabb, T, min_near)
        N = o.shape[0]
        C = self.num_semantic_classes
        dev = o.device
        image = torch.empty(N, 3, device=dev)
        depth = torch.empty(N, device=dev)
        sem = torch.empty(N, C, device=dev)
        chunk, image_width = self.infer_chunk(N, image_width, T + t)
        n_chunks = (N + chunk - 1) // chunk
        if self.hip_pipeline and n_chunks >= 2 and int(self.hip_streams) <= 1:
            # ONE call for the whole batch: density half of chunk k+1 next to
            # the shading half of chunk k (ucsa_render_view; bit-identical)
            ws = self._workspace(
                ops.render_workspace_bytes(min(N, chunk), T, t, f["grid"].n_levels), dev, 2)
            ops.render_view(row.view, f["grid"], f["table"], f["packed_sigma"],
                            f["packed_color"], f["packed_sem"], o, d, nrm, aabb, min_near,
                            rng_t, rng_u, T, t, C, float(self.density_scale), image, depth,
                            sem, chunk, ws[0], ws[1], image_width)
            if self.precision == "f16x2":
                self._h2_finish_render()
            return image, depth, sem
        n_str = max(1, min(int(self.hip_streams), n_chunks))
        ws = self._workspace(
            ops.render_workspace_bytes(min(N, chunk), T, t, f["grid"].n_levels),
            dev, n_str)
        main = torch.cuda.current_stream(dev)
        if n_str > 1:
            while len(self._side_streams) < n_str - 1:
                self._side_streams.append(torch.cuda.Stream(device=dev))
            streams = [main] + self._side_streams[:n_str - 1]
            for st in streams[1:]:
                st.wait_stream(main)  # inputs / packed weights are ready
        else:
            streams = [main]
        render = getattr(ops, row.render)
        for k, head in enumerate(range(0, N, chunk)):
            tail = min(head + chunk, N)
            with torch.cuda.stream(streams[k % n_str]):
                render(
                    f["grid"], f["table"], f["packed_sigma"], f["packed_color"],
                    f["packed_sem"], o[head:tail], d[head:tail], nrm[head:tail],
                    aabb, min_near,
                    None if rng_t is None else rng_t[head:tail],
                    None if rng_u is None else rng_u[head:tail], T, t, C,
                    float(self.density_scale), image[head:tail],
                    depth[head:tail], sem[head:tail], ws[k % n_str],
                    image_width)
        for st in streams[1:]:
            main.wait_stream(st)
        if self.precision == "f16x2":
            self._h2_finish_render()
        return image, depth, sem

    def _run_train(self, o, d, nrm, aabb, T, t, rng_t, rng_u, min_near):
        """Differentiable pass: the same staged kernels with their
        intermediates kept for the backward (see _RenderFn)."""
        return self._render_fn()(self, o, d, nrm, aabb, T, t, rng_t, rng_u,
                                 min_near)

    def _render_fn(self):
        raise NotImplementedError

    def render(self, rays_o, rays_d, direction_norms, staged=False,
               max_ray_batch=4096, bg_color=None, perturb=False, epoch=None,
               **kwargs):
        """reference :301-358.  The reference's ``staged`` loop over
        ``max_ray_batch``-ray chunks only bounds memory; rays are independent,
        so here ``run`` chunks internally (``hip_ray_chunk``) and one call
        covers the whole batch.  Explicit ``rng_t`` / ``rng_u`` are [B,N,*]."""
        # The reference always calls run() (:315); with cuda_ray=True and
        # inference this build marches the occupancy grid instead.
        if self.cuda_ray and (self.march_training or not (
                torch.is_grad_enabled() and self.training)):
            for k in ("num_steps", "upsample_steps", "rng_t", "rng_u"):
                kwargs.pop(k, None)
            return self.run_cuda(rays_o, rays_d, direction_norms,
                                 bg_color=bg_color, perturb=perturb,
                                 epoch=epoch, **kwargs)
        return self.run(rays_o, rays_d, direction_norms=direction_norms,
                        bg_color=bg_color, perturb=perturb, epoch=epoch,
                        **kwargs)
