"""Mirror of reference ``nr4seg/nerf/network_tcnn_semantics.py``.

``SemanticNeRFNetwork`` keeps the reference constructor signature (:12-27),
attribute names (``encoder``, ``sigma_net``, ``encoder_dir``, ``color_net``,
``semantics_net``) and methods (``forward``, ``density``, ``color``,
``semantics``); the tiny-cuda-nn objects are replaced by parameter holders
whose arithmetic runs in the HIP kernels.
"""
from __future__ import annotations

import numpy as np
import os
from typing import NamedTuple

import torch

from .. import _lib, ops
from .encoding import FullyFusedMLP, HashGridEncoding, SHEncoding
from .renderer_semantics import SemanticNeRFRenderer


NETS = {"sigma": "sigma_net", "color": "color_net", "sem": "semantics_net"}

# pack form -> (ops function, suffix of the cache slot).  The function is a NAME,
# looked up at the call, so that replacing ``ops.NAME`` (lab tools, tests) takes.
PACK_FORMS = {"f32": ("mlp_pack", ""), "t": ("mlp_pack_t", "_t"),
              "h": ("mlp_pack_f16", "_h"), "th": ("mlp_pack_t_f16", "_th"),
              "x3": ("mlp_pack_x3", "_x3"), "t_x3": ("mlp_pack_t_x3", "_t_x3"),
              "h2": ("mlp_pack_h2", "_h2")}

# A pack is named (form, net); forms "r16" / "r16_t": _pack_rounded_sigma.
_F32_BWD = dict(packed_color=("f32", "color"), packed_sem=("f32", "sem"),
                packed_color_t=("t", "color"), packed_sem_t=("t", "sem"),
                packed_sigma=("f32", "sigma"), packed_sigma_t=("t", "sigma"))
_F16_BWD = dict(_F32_BWD, packed_color=("h", "color"), packed_sem=("h", "sem"),
                packed_color_t=("th", "color"), packed_sem_t=("th", "sem"))
_X2_BWD = dict(packed_color=("x3", "color"), packed_sem=("x3", "sem"),
               packed_color_t=("t_x3", "color"), packed_sem_t=("t_x3", "sem"),
               packed_sigma=("x3", "sigma"), packed_sigma_t=("t_x3", "sigma"))
# what _field_f16(transposed=True) packs, in its order
_F16_SET = (("h", "sigma"), ("h", "color"), ("h", "sem"), ("th", "color"), ("th", "sem"))
_FUSED_PACKS = tuple((form, name) for form in ("x3", "t_x3", "h2") for name in NETS)


class _TrainPlan(NamedTuple):
    """What one training pass through ``_RenderFn`` runs: decided once, by
    ``_train_plan``, read by the forward and the backward."""
    fused: bool = False          # forward and backward as ONE C call each
    fused_packs: tuple = ()      # ... over these packs (ops.train_packs order)
    half: bool = False           # colour / semantics nets on f16 MFMA
    tcnn: bool = False           # tiny-cuda-nn's numerics end to end
    x2: bool = False             # the backward's contractions as bf16 two-term splits
    half_table: bool = False     # the hash grid read from the table's fp16 copy
    sigma_fwd: str = ""          # ops.sigma_mlp_fwd* and the pack it reads
    sigma_pack: tuple = ()
    shade_fwd: str = ""          # the composite op, its colour / semantics packs, keywords
    shade_packs: tuple = ()
    shade_kw: dict = {}
    bwd: dict = {}               # argument of the backward ops -> pack
    # packs refreshed before the sigma pass / before the shade although that stage
    # does not read them (all of them, or some): the order of the launches is kept
    warm_sigma: tuple = ()
    warm_shade: tuple = ()


def _train_plan(net, t: int) -> _TrainPlan:
    prec = net.train_precision
    x3 = prec == "bf16x3"
    # (round 4) the backward's contractions on the bf16 pipe as two-term splits
    # (2^-16 per product; `nerf: {bwd_precision: fp32}` keeps the f32-input MFMA
    # kernels)
    x2 = x3 and net.bwd_precision == "bf16x2" and ops.shade_bwd_split()
    fwd = "h2" if net.train_fwd_f16x2 else "x3"
    if (x2 and not net.deterministic and net.fused_train_calls and net.grid_records_packed
            and (net.grid_bwd_merged or t == 0)):
        # the default training mode: forward and backward are ONE C call each
        # (ucsa_render_fused_fwd / _bwd: the same launches as the staged passes,
        # sequenced in the library); forward nets as f16x2 (three passes instead
        # of six) with train_fwd_f16x2
        # (no f32 weight packs in this mode: six small launches less per step)
        return _TrainPlan(fused=True, x2=True,
                          fused_packs=_FUSED_PACKS if fwd == "h2" else _FUSED_PACKS[:6])
    if x3:
        # sigma net: fp32-grade on the bf16 pipe, like the colour / semantics
        # forward (1e-7 from the f32-input MFMA chain, 0.04 instead of 0.07 ms per
        # million samples).  Forward of the colour / semantics stage on the split
        # pair with the bf16x3 nets (fp32-grade, the dense bf16 MFMA pipe): same
        # values as the f32-input MFMA chain to ~1e-7; the backward recomputes the
        # nets with the f32-input MFMA as before, or (x2) from the bf16 packs
        return _TrainPlan(
            x2=x2, sigma_fwd="sigma_mlp_fwd_" + fwd, sigma_pack=(fwd, "sigma"),
            shade_fwd="composite_train_fwd_x3", shade_packs=((fwd, "color"), (fwd, "sem")),
            shade_kw=dict(h2=fwd == "h2"), warm_shade=(("x3", "color"), ("x3", "sem")),
            bwd=_X2_BWD if x2 else _F32_BWD)
    # train_precision="fp16": the colour / semantics nets (forward and
    # backward) on f16 MFMA; the sigma net and the hash grid stay fp32
    half = prec in ("fp16", "tcnn")
    plan = _TrainPlan(
        half=half, sigma_fwd="sigma_mlp_fwd", sigma_pack=("f32", "sigma"),
        shade_fwd="composite_fwd", shade_kw=dict(want_aux=True, half=half),
        shade_packs=(("h", "color"), ("h", "sem")) if half else (("f32", "color"), ("f32", "sem")),
        bwd=_F16_BWD if half else _F32_BWD, warm_shade=_F16_SET if half else ())
    if prec != "tcnn":
        return plan
    # train_precision="tcnn": tiny-cuda-nn's numerics end to end -- the
    # hash table read from its fp16 copy, fp16 features, all three nets on
    # f16 MFMA (fp16 weights / layer inputs, fp32 accumulate), half2 bin
    # records; the fp32 parameters are the optimizer's master copy, as in
    # tcnn (network_tcnn_semantics.py:36-58 of the reference).
    # The sigma net's backward runs the fp32 kernel on the forward's
    # fp16-rounded operands (rounded weights, rounded features; fp32
    # accumulation like the f16 MFMA) with the recomputed hidden layer
    # rounded to fp16 as tcnn's forward stored it (round 4:
    # ucsa_sigma_mlp_bwd_h16)
    return plan._replace(
        tcnn=True, half_table=True, sigma_fwd="sigma_mlp_fwd_f16", sigma_pack=("h", "sigma"),
        warm_sigma=_F16_SET, warm_shade=(("r16", "sigma"),),
        bwd=dict(_F16_BWD, packed_sigma=("r16", "sigma"), packed_sigma_t=("r16_t", "sigma")))


class _RenderFn(torch.autograd.Function):
    """Autograd boundary of the HIP renderer.  Differentiable inputs are the
    four flat parameter tensors only (rays, depths and the resampled depths
    carry no gradient in the reference either: new_z_vals is detached,
    renderer_semantics.py:203-207)."""

    @staticmethod
    def forward(ctx, grid_p, sigma_p, color_p, sem_p, net, o, d, nrm, aabb, T,
                t, rng_t, rng_u, min_near):
        N = o.shape[0]
        C = net.num_semantic_classes
        ds = float(net.density_scale)
        plan = _train_plan(net, t)
        ctx.plan, ctx.net, ctx.aabb, ctx.T, ctx.t = plan, net, aabb, T, t
        if plan.fused:
            pk = [net._pack(form, name) for form, name in plan.fused_packs]
            f = dict(grid=net.encoder.grid, table=net.encoder.params.detach())
            image, depth, sem, sv = ops.render_fused_fwd(
                f["grid"], f["table"], ops.train_packs(*pk), o, d, nrm, aabb, min_near,
                rng_t, rng_u, T, t, C, ds)
            ctx.f, ctx.pk, ctx.sv, ctx.rays = f, pk, sv, (o, d, nrm)
            return image, depth, sem
        f32 = net._field(transposed=True)
        near, far = ops.near_far_from_aabb(o, d, aabb, min_near)
        z_c = ops.sample_coarse(near, far, T, rng_t)
        net._build(plan.warm_sigma)
        table = net._table_half() if plan.half_table else f32["table"]
        sig_fwd, sig_pack = getattr(ops, plan.sigma_fwd), net._pack(*plan.sigma_pack)
        feat_c = ops.hashgrid_encode_rays(f32["grid"], table, o, d, z_c, aabb)
        h_c, s_c = sig_fwd(feat_c, sig_pack)
        s_c = s_c.view(N, T)
        if t > 0:
            z_f = ops.resample(z_c, s_c, rng_u, ds)
            feat_f = ops.hashgrid_encode_rays(f32["grid"], table, o, d, z_f, aabb)
            h_f, s_f = sig_fwd(feat_f, sig_pack)
            s_f = s_f.view(N, t)
        else:
            z_f = feat_f = h_f = s_f = None
        net._build(plan.warm_shade)
        image, depth, sem, src, w = getattr(ops, plan.shade_fwd)(
            d, nrm, z_c, s_c, h_c, z_f, s_f, h_f, net._pack(*plan.shade_packs[0]),
            net._pack(*plan.shade_packs[1]), C, ds, **plan.shade_kw)
        # the backward's packs, stale ones made now, in this order
        ctx.f = dict(grid=f32["grid"], **{k: net._pack(*fn) for k, fn in plan.bwd.items()})
        ctx.saved = (o, d, nrm, z_c, feat_c, h_c, s_c, z_f, feat_f, h_f, s_f,
                     src, w)
        return image, depth, sem

    @staticmethod
    def backward(ctx, d_image, d_depth, d_sem):
        net, f, aabb, T, t, plan = ctx.net, ctx.f, ctx.aabb, ctx.T, ctx.t, ctx.plan
        if plan.fused:
            o, d, nrm = ctx.rays
            g_grid = torch.zeros_like(net.encoder.params)
            g_sigma = torch.empty_like(net.sigma_net.params)
            g_color = torch.empty_like(net.color_net.params)
            g_sem = torch.empty_like(net.semantics_net.params)
            ops.render_fused_bwd(f["grid"], ops.train_packs(*ctx.pk), o, d, nrm, aabb, ctx.sv,
                                 d_image.contiguous(), d_depth.contiguous(), d_sem.contiguous(),
                                 net.num_semantic_classes, float(net.density_scale),
                                 g_grid, g_sigma, g_color, g_sem)
            ctx.sv = ctx.pk = ctx.rays = None
            return (g_grid, g_sigma, g_color, g_sem) + (None,) * 10
        (o, d, nrm, z_c, feat_c, h_c, s_c, z_f, feat_f, h_f, s_f, src,
         w) = ctx.saved
        C = net.num_semantic_classes
        ds = float(net.density_scale)
        d_h_c, d_h_f, pc, ps = ops.composite_bwd(
            d, nrm, z_c, s_c, h_c, z_f, s_f, h_f, src, w, f["packed_color"],
            f["packed_sem"], f["packed_color_t"], f["packed_sem_t"],
            d_image.contiguous(), d_depth.contiguous(), d_sem.contiguous(), C,
            ds, half=plan.half, f16_scale=float(net.f16_bwd_scale), x2=plan.x2)
        g_color = torch.empty_like(net.color_net.params)
        g_sem = torch.empty_like(net.semantics_net.params)
        ops.reduce_partials(pc, g_color, False)
        ops.reduce_partials(ps, g_sem, False)
        g_sigma = torch.empty_like(net.sigma_net.params)
        g_grid = torch.zeros_like(net.encoder.params)
        if plan.tcnn:   # fp16 features -> the fp32 kernel's operand type
            feat_c = feat_c.float()
            feat_f = None if feat_f is None else feat_f.float()
        d_feat, part = ops.sigma_mlp_bwd(feat_c, d_h_c, f["packed_sigma"],
                                         f["packed_sigma_t"], x2=plan.x2,
                                         round_hidden=plan.tcnn)
        ops.reduce_partials(part, g_sigma, False)
        # f16 training mode: 8-byte bin records (half2 values under the same
        # loss scale as the nets' gradient operands)
        rs = float(net.f16_bwd_scale) if (plan.half and (net.f16_grid_records or plan.tcnn)) else 0.0
        merged = t > 0 and net.grid_bwd_merged
        # bf16x2 backward: 8-byte packed bin records (26-bit values, 2^-18 --
        # finer than the two-term split that produced them)
        pk = plan.x2 and rs == 0.0 and net.grid_records_packed
        if net.deterministic:
            # `UCSA_DETERMINISTIC=1` / net.deterministic: order-independent
            # fixed-point accumulation of the table gradient (two runs of a step
            # give the same bits; ucsa_hashgrid_bwd_rays_det)
            fix = ops.hashgrid_bwd_rays_det(f["grid"], o, d, z_c, aabb, d_feat)
            if t > 0:
                d_feat_f, part = ops.sigma_mlp_bwd(feat_f, d_h_f, f["packed_sigma"],
                                                   f["packed_sigma_t"], x2=plan.x2,
                                                   round_hidden=plan.tcnn)
                ops.reduce_partials(part, g_sigma, True)
                ops.hashgrid_bwd_rays_det(f["grid"], o, d, z_f, aabb, d_feat_f, fix)
            ops.hashgrid_bwd_det_finish(f["grid"], fix, g_grid)
            ctx.saved = None
            return (g_grid, g_sigma, g_color, g_sem) + (None,) * 10
        if not merged:
            ops.hashgrid_bwd_rays(f["grid"], o, d, z_c, aabb, d_feat, g_grid,
                                  rec_scale=rs, packed=pk)
        if t > 0:
            d_feat_f, part = ops.sigma_mlp_bwd(feat_f, d_h_f, f["packed_sigma"],
                                               f["packed_sigma_t"], x2=plan.x2,
                                               round_hidden=plan.tcnn)
            ops.reduce_partials(part, g_sigma, True)
            if merged:
                # both passes in one call, the ray's samples in sorted order: the
                # fine samples join the coarse samples' runs on the coarse levels
                ops.hashgrid_bwd_rays_merged(f["grid"], o, d, z_c, z_f, src, aabb,
                                             d_feat, d_feat_f, g_grid, packed=pk,
                                             rec_scale=rs)
            else:
                ops.hashgrid_bwd_rays(f["grid"], o, d, z_f, aabb, d_feat_f, g_grid,
                                      rec_scale=rs, packed=pk)
        ctx.saved = None
        return (g_grid, g_sigma, g_color, g_sem) + (None,) * 10


class _MarchRenderFn(torch.autograd.Function):
    """Autograd boundary of the marched training pass:
    occupancy-grid samples (ucsa_march_rays_train) -> hash grid + sigma MLP on
    the points -> fused weights / compaction / colour + semantics nets /
    compositing (ucsa_march_train_fwd), and the matching backward.  As in
    ``_RenderFn`` only the four parameter tensors are differentiable."""

    @staticmethod
    def forward(ctx, grid_p, sigma_p, color_p, sem_p, net, o, d, nrm, nears,
                xyzs, deltas, rays, w_min):
        f = net._field(transposed=True)
        C = net.num_semantic_classes
        ds = float(net.density_scale)
        M = xyzs.shape[0]
        feat = ops.hashgrid_encode_points(f["grid"], f["table"], xyzs)
        h, sigma = ops.sigma_mlp_fwd(feat, f["packed_sigma"])
        ws, depth_raw, image, sem, w, t = ops.march_train_fwd(
            rays, M, nears, d, sigma, ds, h, deltas, f["packed_color"],
            f["packed_sem"], C, w_min)
        ctx.net, ctx.f, ctx.w_min = net, f, w_min
        ctx.saved = (d, nrm, xyzs, deltas, rays, feat, h, sigma, w, t)
        ctx.mark_non_differentiable(ws)
        return image, depth_raw / nrm, sem, ws

    @staticmethod
    def backward(ctx, d_image, d_depth, d_sem, _d_ws):
        net, f, w_min = ctx.net, ctx.f, ctx.w_min
        d, nrm, xyzs, deltas, rays, feat, h, sigma, w, t = ctx.saved
        C = net.num_semantic_classes
        M = xyzs.shape[0]
        d_h, pc, ps = ops.march_train_bwd(
            rays, M, d, nrm, sigma, float(net.density_scale), h, deltas, w, t,
            f["packed_color"], f["packed_sem"], f["packed_color_t"],
            f["packed_sem_t"], C, w_min, d_image.contiguous(),
            d_depth.contiguous(), d_sem.contiguous())
        g_color = torch.empty_like(net.color_net.params)
        g_sem = torch.empty_like(net.semantics_net.params)
        g_sigma = torch.zeros_like(net.sigma_net.params)
        g_grid = torch.zeros_like(net.encoder.params)
        pairs = [(pc, g_color), (ps, g_sem)]
        if M > 0:
            d_feat, part = ops.sigma_mlp_bwd(feat, d_h, f["packed_sigma"],
                                             f["packed_sigma_t"])
            pairs.append((part, g_sigma))
            ops.hashgrid_bwd_points(f["grid"], xyzs, d_feat, g_grid)
        ops.reduce_partials_multi(pairs)   # one launch for the three MLPs
        ctx.saved = None
        return (g_grid, g_sigma, g_color, g_sem) + (None,) * 9


class SemanticNeRFNetwork(SemanticNeRFRenderer):

    def __init__(self, encoding="HashGrid", encoding_dir="SphericalHarmonics",
                 num_layers=2, hidden_dim=64, geo_feat_dim=15,
                 num_layers_color=3, hidden_dim_color=64,
                 num_layers_semantics=2, hidden_dim_semantics=64, bound=1,
                 num_semantic_classes=41, seed=None, **kwargs):
        super().__init__(bound, **kwargs,
                         num_semantic_classes=num_semantic_classes)
        if (num_layers, num_layers_color, num_layers_semantics,
                geo_feat_dim) != (2, 3, 2, 15):
            raise ValueError(
                "the HIP kernels implement the reference configuration: "
                "sigma 32->64->16, colour 32->64->64->3, semantics 16->64->C")
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.geo_feat_dim = geo_feat_dim
        gen = torch.Generator().manual_seed(seed) if seed is not None else None

        # reference :34
        per_level_scale = float(np.exp2(np.log2(2048 * bound / 16) / (16 - 1)))
        self.encoder = HashGridEncoding(bound, 16, 2, 19, 16, per_level_scale,
                                        seed=seed)
        self.sigma_net = FullyFusedMLP(32, 1 + geo_feat_dim, hidden_dim,
                                       num_layers - 1, _lib.MLP_SIGMA, gen)
        self.num_layers_color = num_layers_color
        self.hidden_dim_color = hidden_dim_color
        self.encoder_dir = SHEncoding(4)
        self.in_dim_color = self.encoder_dir.n_output_dims + geo_feat_dim
        self.color_net = FullyFusedMLP(self.in_dim_color, 3, hidden_dim_color,
                                       num_layers_color - 1, _lib.MLP_COLOR,
                                       gen)
        self.num_layers_semantics = num_layers_semantics
        self.hidden_dim_semantics = hidden_dim_semantics
        self.in_dim_semantics = geo_feat_dim
        self.semantics_net = FullyFusedMLP(geo_feat_dim, num_semantic_classes,
                                           hidden_dim_semantics,
                                           num_layers_semantics - 1,
                                           _lib.MLP_SEM, gen)
        self._packed = {}
        # f16x2 range guard (VERDICT r4 item 5 / ADVICE r4): "weights" (default)
        # checks max|W| of a net whenever its f16x2 pack is refreshed, "full" also
        # the activations of a sample of every no-grad render, "off" nothing.
        # UCSA_H2_GUARD overrides.
        self.h2_guard = "weights"
        self._h2_seen = {}
        self._h2_eval_pending = False
        self._h2_flags = {}
        self._h2_scratch = {}
        # reproducibility mode: the hash-grid gradient through an
        # order-independent fixed-point reduction instead of float atomics / bin
        # records -- two runs of a training step then give the same bits.  ~8 x
        # slower backward: for debugging and for the trajectory-parity test.
        self.deterministic = os.environ.get("UCSA_DETERMINISTIC", "0") == "1"

    def __getstate__(self):
        """copy.deepcopy / pickle of the module: per-process runtime state stays
        behind -- streams and events cannot be copied, and the render workspaces
        (gigabytes of scratch) and pinned read-back slots should not be."""
        st = dict(self.__dict__)
        st.update(_h2_eval_pending=False, _h2_flags={}, _h2_scratch={}, _h2_seen={},
                  _side_streams=[], _ws=None)
        return st

    # f16x2's first terms are f16 and ucsa_mlp_pack_h2 stores the last layer
    # times 2^4: a weight of 65504 / 16 or more becomes inf, the two partial sums
    # give inf - inf = NaN and a NaN pre-activation passes ReLU as 0 -- silently
    # (csrc/mfma_mlp_h2.h).  The guard makes that loud.
    H2_INPUT_LIMIT = 65504.0
    H2_HIDDEN_LIMIT = float(2 ** 20)

    def _h2_guard_mode(self) -> str:
        mode = os.environ.get("UCSA_H2_GUARD", "") or self.h2_guard
        if mode not in ("off", "weights", "full"):
            raise ValueError(f"h2_guard / UCSA_H2_GUARD must be off, weights or full, got {mode!r}")
        return mode

    def _h2_fail(self, name: str, amax: float):
        raise _lib.UcsaError(
            f"f16x2 nets: the {name} net holds a weight that packs to {amax!r} (first / last "
            "layer scaled by 2^-4 / 2^4), outside the range of precision 'f16x2' (< 65504, "
            "finite; csrc/mfma_mlp_h2.h): the kernels would turn the overflow into zeros "
            "silently.  Use nerf: {precision: bf16x3} (fp32 range) for this field.")

    H2_BITS_LIMIT = 0x477FE000     # 65504.0f as an fp32 bit pattern

    def _h2_flag(self, name: str, device):
        """The net's range word: ONE int32 of pinned host memory that the device
        addresses directly (ucsa_mlp_pack_h2_checked raises it with a system-scope
        atomic max, nothing lowers it).  The host reads it like any memory."""
        f = self._h2_flags.get(name)
        if f is None:
            f = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._h2_flags[name] = f
        return f

    def _h2_poll(self, block: bool = False):
        """Raise if a net's range word shows an out-of-range pack.  ``block``:
        wait for the device first, so that every pack launched so far is in."""
        if block and torch.cuda.is_available():
            torch.cuda.synchronize()
        for name, f in self._h2_flags.items():
            bits = int(f[0]) & 0xFFFFFFFF
            if bits >= self.H2_BITS_LIMIT:
                import struct
                f.zero_()                      # reported once: both words start over
                if name in self._h2_scratch:
                    self._h2_scratch[name].zero_()
                self._h2_fail(name, struct.unpack("<f", struct.pack("<I", bits))[0])

    def _h2_after_pack(self, name: str):
        """The range guard's host side (`h2_guard: weights`, the default).  The
        pack kernel itself keeps the largest |value| it converted to f16 in the
        net's word in pinned host memory -- no launch, allocation, copy, stream,
        event or wait per pack (round 5 measured every one of those: a blocking
        read between the pack launches made each later training step of the
        process 0.15 ms slower; a norm + copy per pack, and even one more stream in
        the process, the joint step 177 -> 231-245 ms).  The word only grows and
        the host can read it at any time: it looks at every pack (a memory read; a
        pack launched a few steps ago has landed by then), and a net packed for
        the FIRST time in this process -- a loaded checkpoint -- is judged before
        its first render returns (``_h2_finish_render``)."""
        n = self._h2_seen.get(name, 0)
        self._h2_seen[name] = n + 1
        self._h2_poll()
        if n == 0 and not (self.training and torch.is_grad_enabled()):
            self._h2_eval_pending = True

    def _h2_finish_render(self):
        """End of a no-grad render that packed a net for the first time: wait for
        the device and raise before the outputs are returned."""
        if self._h2_eval_pending:
            self._h2_eval_pending = False
            self._h2_poll(block=True)

    def _h2_check_activations(self, o, d, aabb, T, min_near):
        """h2_guard "full": the layer inputs and hidden activations of a sample
        of the render's rays against f16x2's range -- the sigma net evaluated
        in plain fp32 torch on the coarse samples of <= 2048 rays, the colour /
        semantics nets through a row-norm bound on their hidden layers."""
        with torch.no_grad():
            step = max(1, o.shape[0] // 2048)
            oo, dd = o[::step].contiguous(), d[::step].contiguous()
            near, far = ops.near_far_from_aabb(oo, dd, aabb, min_near)
            z = ops.sample_coarse(near, far, min(int(T), 64))
            feat = ops.hashgrid_encode_rays(self.encoder.grid, self.encoder.params.detach(),
                                            oo, dd, z, aabb)
            x = feat.permute(1, 0, 2).reshape(feat.shape[1], -1)
            ws = self.sigma_net.params.detach()
            (r1, c1), (r2, c2) = self.sigma_net.shapes
            w1, w2 = ws[:r1 * c1].view(r1, c1), ws[r1 * c1:r1 * c1 + r2 * c2].view(r2, c2)
            hid = torch.relu(x @ w1.t())
            out = hid @ w2.t()
            found = {"hash-grid features (sigma net input)": (float(x.abs().max()), self.H2_INPUT_LIMIT),
                     "sigma net hidden layer": (float(hid.max()), self.H2_HIDDEN_LIMIT),
                     "sigma net output (geo_feat, colour / semantics input)":
                         (float(out.abs().max()), self.H2_INPUT_LIMIT)}
            bound = max(float(out.abs().max()), 1.0)     # SH basis and the padding are <= 1
            for name, net in (("colour", self.color_net), ("semantics", self.semantics_net)):
                off = 0
                for li, (r, c) in enumerate(net.shapes[:-1]):
                    w = net.params.detach()[off:off + r * c].view(r, c)
                    off += r * c
                    bound = float(w.abs().sum(dim=1).max()) * bound   # >= any activation
                    found[f"{name} net hidden layer {li + 1} (row-norm bound)"] = (bound, self.H2_HIDDEN_LIMIT)
                bound = max(float(out.abs().max()), 1.0)
        for what, (v, lim) in found.items():
            if not v < lim:
                raise _lib.UcsaError(
                    f"f16x2 nets: {what} reaches {v!r}, outside the range of precision "
                    f"'f16x2' (< {lim:g}; csrc/mfma_mlp_h2.h).  Use nerf: {{precision: bf16x3}}.")

    # -- packed (MFMA A-fragment order) weights, refreshed when params change
    def _cached(self, slot: str, p, make, *args):
        """``self._packed[slot]``: what ``make(out, *args)`` made of the parameter
        ``p``, made again when ``p`` was written to or replaced -- into the old
        buffer (``out``) unless ``p`` moved to another device (``out`` None)."""
        key = (p.data_ptr(), p._version)
        hit = self._packed.get(slot)
        here = hit is not None and (hit[1][0] if isinstance(hit[1], tuple) else hit[1]).device == p.device
        if not here or hit[0] != key:
            self._packed[slot] = (key, make(hit[1] if here else None, *args))
            return self._packed[slot][1], True
        return hit[1], False

    def _pack(self, form: str, name: str):
        """The net ``name`` (NETS) packed in ``form`` (PACK_FORMS)."""
        if form in ("r16", "r16_t"):
            return self._pack_rounded_sigma()[form == "r16_t"]
        net = getattr(self, NETS[name])
        packed, fresh = self._cached(name + PACK_FORMS[form][1], net.params, self._make_pack,
                                     form, name, net)
        if fresh and form == "h2" and self._h2_guard_mode() != "off":
            self._h2_after_pack(name)
        return packed

    def _make_pack(self, out, form, name, net):
        p, kw = net.params, {}
        if form == "h2":
            # weights as two f16 terms (csrc/mfma_mlp_h2.h); under the range guard
            # the pack kernel keeps max|value| in the net's pinned range word
            guard = self._h2_guard_mode() != "off"
            if guard and (name not in self._h2_scratch or self._h2_scratch[name].device != p.device):
                self._h2_scratch[name] = torch.zeros(2, dtype=torch.int32, device=p.device)
            kw = dict(range_bits=self._h2_flag(name, p.device) if guard else None,
                      scratch=self._h2_scratch.get(name) if guard else None)
        return getattr(ops, PACK_FORMS[form][0])(net.kind, p, self.num_semantic_classes,
                                                  out=out, **kw)

    def _build(self, packs):
        for form, name in packs:
            self._pack(form, name)

    def _pack_rounded_sigma(self):
        """fp32 packs (forward and transposed) of the sigma net's weights
        ROUNDED to fp16: what the f16 forward multiplied with, for the fp32
        backward kernel of train_precision="tcnn"."""
        return self._cached("sigma_r16", self.sigma_net.params, self._make_rounded_sigma)[0]

    def _make_rounded_sigma(self, out):
        r = self.sigma_net.params.detach().half().float()
        return (ops.mlp_pack(self.sigma_net.kind, r, self.num_semantic_classes),
                ops.mlp_pack_t(self.sigma_net.kind, r, self.num_semantic_classes))

    def _table_half(self):
        """fp16 copy of the hash table (what tiny-cuda-nn stores), refreshed
        when the fp32 parameters change."""
        return self._cached("table_h16", self.encoder.params, self._make_table_half)[0]

    def _make_table_half(self, out):
        return ops.table_to_half(self.encoder.params, out=out)

    def _nets(self, form: str, transposed: bool = False):
        """grid, table and the three nets packed in ``form``; ``transposed``: also
        the transposed packs (``form`` "f32": all three, "h": colour and
        semantics, which is what their backward kernels read)."""
        f = dict(grid=self.encoder.grid, table=self.encoder.params.detach())
        for name in NETS:
            f["packed_" + name] = self._pack(form, name)
        if transposed:
            t_form = {"f32": "t", "h": "th"}[form]
            for name in (NETS if form == "f32" else ("color", "sem")):
                f["packed_" + name + "_t"] = self._pack(t_form, name)
        return f

    def _field_x3(self):
        """Weights as three bf16 terms each (csrc/mfma_mlp_x3.h)."""
        return self._nets("x3")

    def _field_h2(self):
        """Weights as two f16 terms each (csrc/mfma_mlp_h2.h, "f16x2")."""
        return self._nets("h2")

    def _field_f16(self, transposed: bool = False):
        return self._nets("h", transposed)

    def _field(self, transposed: bool = False):
        return self._nets("f32", transposed)

    def _render_fn(self):
        def call(net, o, d, nrm, aabb, T, t, rng_t, rng_u, min_near):
            return _RenderFn.apply(net.encoder.params, net.sigma_net.params,
                                   net.color_net.params,
                                   net.semantics_net.params, net, o, d, nrm,
                                   aabb, T, t, rng_t, rng_u, min_near)
        return call

    def _march_render_fn(self):
        def call(net, o, d, nrm, nears, xyzs, deltas, rays, w_min):
            if net.deterministic and torch.is_grad_enabled():
                # the marched backward sums the table gradient with float
                # atomics; silently ignoring the request would defeat its purpose
                raise _lib.UcsaError("UCSA_DETERMINISTIC=1 / net.deterministic covers the "
                                     "uniform-sampling training path only; the marched "
                                     "(cuda_ray=True) backward has no order-independent "
                                     "table reduction")
            return _MarchRenderFn.apply(net.encoder.params,
                                        net.sigma_net.params,
                                        net.color_net.params,
                                        net.semantics_net.params, net, o, d,
                                        nrm, nears, xyzs, deltas, rays, w_min)
        return call

    # -- pointwise API (reference :102-207) -----------------------------------
    def density(self, x):
        """x [M,3] in [-bound,bound] -> {"sigma" [M], "geo_feat" [M,15]}."""
        f = self._field()
        with torch.no_grad():
            feat = ops.hashgrid_encode_points(f["grid"], f["table"], x)
            h, sigma = ops.sigma_mlp_fwd(feat, f["packed_sigma"])
        return {"sigma": sigma, "geo_feat": h[:, 1:]}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """reference :147-178.  x is unused by the colour net (as in the
        reference, where only d and geo_feat feed it).  Inference only."""
        f = self._field()
        with torch.no_grad():
            rgb, _ = ops.point_shade(d, geo_feat, mask, f["packed_color"],
                                     f["packed_sem"],
                                     self.num_semantic_classes,
                                     want_probs=False)
        return rgb

    def semantics(self, x, d, mask=None, geo_feat=None, **kwargs):
        """reference :180-207: softmax probabilities, zero rows outside the
        mask.  Inference only."""
        f = self._field()
        with torch.no_grad():
            _, probs = ops.point_shade(None, geo_feat, mask, f["packed_color"],
                                       f["packed_sem"],
                                       self.num_semantic_classes,
                                       want_rgb=False)
        return probs

    def forward(self, x, d):
        """reference :102-128 -> (sigma [M], color [M,3], semantics [M,C])."""
        den = self.density(x)
        geo = den["geo_feat"].contiguous()
        return (den["sigma"], self.color(x, d, geo_feat=geo),
                self.semantics(x, d, geo_feat=geo))

    # -- labelled-mesh export (not in the reference; its parent code base,
    # torch-ngp, had extract_geometry / save_mesh on the CPU) -----------------
    LATTICE_SLAB_POINTS = 1 << 22

    def _lattice_frame(self, resolution, aabb):
        res = ((int(resolution),) * 3 if np.isscalar(resolution)
               else tuple(int(r) for r in resolution))
        if len(res) != 3 or min(res) < 2:
            raise ValueError(f"resolution must be >= 2 per axis, got {resolution}")
        box = self.aabb_infer if aabb is None else aabb
        box = torch.as_tensor(box, dtype=torch.float32).detach().cpu().reshape(6)
        lo, hi = box[:3], box[3:]
        spacing = (hi - lo) / torch.tensor([r - 1 for r in res], dtype=torch.float32)
        return res, lo, spacing

    @torch.no_grad()
    def density_lattice(self, resolution, aabb=None):
        """sigma on a dense lattice [nx,ny,nz] (``resolution``: an int or three),
        as ``density()`` returns it.  Point (i,j,k) sits at lo + (i,j,k)*spacing
        (fp32), lo / hi = ``aabb`` [6] (default ``aabb_infer``), spacing =
        (hi - lo) / (resolution - 1), so the lattice spans the box corner to
        corner.  Runs in slabs of whole (y,z) planes through
        ``ops.hashgrid_encode_points`` + ``ops.sigma_mlp_fwd``, at most
        ``LATTICE_SLAB_POINTS`` (4 Mi) points per slab: the point path keeps
        ~52 floats per point (coordinates, 32 features, 16 outputs, sigma), so the
        scratch peaks near 0.9 GB whatever the resolution; the result itself is
        4 bytes per point (0.54 GB at 512^3)."""
        (nx, ny, nz), lo, h = self._lattice_frame(resolution, aabb)
        dev = self.encoder.params.device
        axes = [(lo[a] + torch.arange(n, dtype=torch.float32) * h[a]).to(dev)
                for a, n in enumerate((nx, ny, nz))]
        out = torch.empty(nx, ny, nz, device=dev)
        plane = ny * nz
        step = max(1, self.LATTICE_SLAB_POINTS // plane)
        yz = torch.stack(torch.meshgrid(axes[1], axes[2], indexing="ij"), -1).reshape(-1, 2)
        for i0 in range(0, nx, step):
            i1 = min(nx, i0 + step)
            xs = axes[0][i0:i1]
            pts = torch.cat([xs.repeat_interleave(plane)[:, None],
                             yz.repeat(i1 - i0, 1)], 1)
            out[i0:i1] = self.density(pts)["sigma"].view(i1 - i0, ny, nz)
        return out

    @torch.no_grad()
    def extract_semantic_mesh(self, resolution=256, threshold=10.0, aabb=None,
                              color=True, chunk=1 << 20):
        """The iso-surface sigma = ``threshold`` of the field as an indexed,
        labelled mesh: a dict of numpy arrays
          verts [V,3] f32, faces [F,3] int32, normals [V,3] f32 (outward, i.e.
          toward lower density; ops.marching_cubes over ``density_lattice``),
          labels [V] int64 in 0..C-1: argmax of ``semantics()`` on the vertex's
          ``geo_feat``,
          rgb [V,3] f32 (``color=True``): ``color()`` seen along -normal, along
          (0,0,1) where the normal is zero.
        Vertices are in the field's (NGP) frame; ``utils.semantic_mesh.
        ngp_to_pose_frame`` maps them into the frame of transforms_train.json.
        Attributes in chunks of ``chunk`` vertices.  Changes nothing: not the
        parameters, the occupancy grid, the counters or the RNG state."""
        res, lo, h = self._lattice_frame(resolution, aabb)
        sigma = self.density_lattice(res, aabb)
        verts, faces, normals = ops.marching_cubes(sigma, float(threshold), lo.tolist(),
                                                   h.tolist())
        del sigma
        V = verts.shape[0]
        labels = torch.empty(V, dtype=torch.int64, device=verts.device)
        rgb = torch.empty(V, 3, device=verts.device) if color else None
        for a in range(0, V, chunk):
            b = min(V, a + chunk)
            geo = self.density(verts[a:b])["geo_feat"].contiguous()
            labels[a:b] = self.semantics(None, None, geo_feat=geo).argmax(-1)
            if color:
                nrm = normals[a:b]
                zero = (nrm == 0).all(-1, keepdim=True)
                view = torch.where(zero, torch.tensor([0.0, 0.0, 1.0], device=nrm.device),
                                   -nrm)
                rgb[a:b] = self.color(None, view.contiguous(), geo_feat=geo)
        out = {"verts": verts, "faces": faces, "normals": normals, "labels": labels}
        if color:
            out["rgb"] = rgb
        return {k: v.cpu().numpy() for k, v in out.items()}
