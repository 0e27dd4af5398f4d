"""The float64 reference of the marched compositing kernels
(tests/march_numpy.py), without a GPU: the fp32 C oracle (oracle/raymarch.c)
passes the element-wise check on every reference-API case; the same formulas
evaluated sequentially in fp32 pass on every case of the GPU test (the bounds
are not tighter than fp32 allows); every deliberate mistake is rejected by a
named case (they are not so wide that a wrong kernel would pass); no builder
redraws more than 5 % of its samples and every placed stop sits where it was
asked for; and the marched training reference agrees with torch autograd on
``_oracle_marched_render`` of tests/test_gpu_raymarch.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import raymarch as orm
from tests import march_numpy as mn
from tests import shade_numpy as sn
from tests.util import lively_oracle_field

F32, F64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def _params(C):
    fld = lively_oracle_field(C=C)
    return fld.color_params.numpy(), fld.sem_params.numpy()


@functools.lru_cache(maxsize=None)
def _train(name):
    c = mn.build_train_case(name)
    return (c,) + mn.train_refs(c)


@functools.lru_cache(maxsize=None)
def _update(name):
    c = mn.build_update_case(name)
    seg = mn.segment_composite(*mn.update_args(c))
    stp = mn.composite_rays_update(*mn.steps_args(c))
    return c, seg, stp


@functools.lru_cache(maxsize=None)
def _fused(name, mode_name="fp32", C=40, w_min=1e-4):
    mode = {"fp32": sn.FP32, "h2": sn.H2, "f16": sn.F16M(1024.0)}[mode_name]
    c = mn.build_fused_case(name, *_params(C), mode, C=C, w_min=w_min)
    return c, mn.segment_shade(*mn.fused_args(c))


@functools.lru_cache(maxsize=None)
def _march(name, C=40, w_min=1e-4):
    c = mn.build_march_train_case(name, *_params(C), C=C, w_min=w_min)
    fw = mn.march_train_forward(*mn.march_fwd_args(c))
    w32, t32 = fw.w_out.astype(F32), fw.t_out.astype(F32)
    return c, fw, w32, t32, mn.march_train_backward(*mn.march_bwd_args(c, w32, t32))


TRAIN = list(mn.train_case_specs())
UPDATE = list(mn.update_case_specs())
FUSED = list(mn.fused_case_specs())
MARCH = list(mn.march_train_specs())


# ---------------------------------------------------------------------------
# the fp32 C oracle within the bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAIN)
def test_oracle_composite_rays_train(name):
    c, fw, bw = _train(name)
    got = orm.composite_rays_train(c.sigmas, c.rgbs, c.deltas, c.rays, c.local_sem)
    got = dict(zip(mn.TRAIN_KEYS, got))
    mn.compare_fields(got, fw, mn.TRAIN_KEYS, "oracle train fwd", name)
    g = orm.composite_rays_train_backward(c.g_ws, c.g_img, c.sigmas, c.rgbs, c.deltas, c.rays,
                                          got["weights_sum"], got["image"], c.g_sem)
    mn.compare_fields(dict(zip(mn.TRAIN_BWD_KEYS, g)), bw, mn.TRAIN_BWD_KEYS, "oracle train bwd", name)
    # rows of dropped and empty spans stay zero, their rays give zeros
    ids = c.rays[c.dropped | (c.rays[:, 2] == 0), 0]
    assert (fw.weights_sum[ids] == 0).all() and (fw.image[ids] == 0).all()
    for off, cnt in c.rays[c.dropped][:, 1:]:
        assert (bw.grad_sigmas[off:off + cnt] == 0).all() and (bw.grad_rgbs[off:off + cnt] == 0).all()


@pytest.mark.parametrize("name", UPDATE)
def test_oracle_composite_rays(name):
    c, _, ref = _update(name)
    n_alive, n_step, ra, rt, sig, rgb, ls, dl = mn.steps_args(c)[:8]
    rt, ws, dep, img = rt.copy(), c.weights_sum.copy(), c.depth.copy(), c.image.copy()
    sem = None if c.semantics is None else c.semantics.copy()
    orm.composite_rays(n_alive, n_step, ra, rt, sig, rgb, dl, ws, dep, img, ls, sem)
    got = dict(weights_sum=ws, depth=dep, image=img, semantics=sem, rays_t=rt)
    mn.compare_fields(got, ref, mn.UPDATE_KEYS, "oracle composite_rays", name)
    assert ((rt[:n_alive] == -1) == ref.finished).all()


# ---------------------------------------------------------------------------
# plain fp32 evaluation within the bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAIN)
def test_fp32_train(name):
    c, fw, bw = _train(name)
    f32, b32 = mn.train_refs(c, dt=F32)
    assert f32.image.dtype == F32 and b32.grad_sigmas.dtype == F32
    mn.compare_fields(mn.as_got(f32, mn.TRAIN_KEYS), fw, mn.TRAIN_KEYS, "fp32 train fwd", name)
    mn.compare_fields(mn.as_got(b32, mn.TRAIN_BWD_KEYS), bw, mn.TRAIN_BWD_KEYS, "fp32 train bwd", name)


@pytest.mark.parametrize("name", UPDATE)
def test_fp32_update(name):
    c, seg, stp = _update(name)
    s32 = mn.segment_composite(*mn.update_args(c), dt=F32)
    assert s32.image.dtype == F32
    mn.compare_fields(mn.as_got(s32, mn.UPDATE_KEYS), seg, mn.UPDATE_KEYS, "fp32 segment_composite", name)
    p32 = mn.composite_rays_update(*mn.steps_args(c), dt=F32)
    mn.compare_fields(mn.as_got(p32, mn.UPDATE_KEYS), stp, mn.UPDATE_KEYS, "fp32 composite_rays", name)
    assert (s32.finished == seg.finished).all() and (p32.finished == stp.finished).all()


@pytest.mark.parametrize("mode", ["fp32", "h2"])
@pytest.mark.parametrize("name", FUSED)
def test_fp32_fused(name, mode):
    c, ref = _fused(name, mode)
    got = mn.segment_shade(*mn.fused_args(c), dt=F32)
    assert (got.sw.keep == ref.sw.keep).all() and (got.finished == ref.finished).all()
    mn.compare_fields(mn.as_got(got, mn.FUSED_KEYS), ref, mn.FUSED_KEYS, "fp32 segment_shade", name)


@pytest.mark.parametrize("name", MARCH)
def test_fp32_march_train(name):
    c, fw, w32, t32, bw = _march(name)
    f32 = mn.march_train_forward(*mn.march_fwd_args(c), dt=F32)
    mn.compare_fields(mn.as_got(f32, mn.MARCH_FWD_KEYS), fw, mn.MARCH_FWD_KEYS, "fp32 march fwd", name)
    b32 = mn.march_train_backward(*mn.march_bwd_args(c, w32, t32), dt=F32)
    mn.compare_fields(mn.as_got(b32, mn.MARCH_BWD_KEYS), bw, mn.MARCH_BWD_KEYS, "fp32 march bwd", name)


# ---------------------------------------------------------------------------
# pinning
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", UPDATE)
def test_update_cases_are_pinned(name):
    c, seg, stp = _update(name)
    for sw, what in ((seg.sw, "segment"), (stp.sw, "steps")):
        mn.check_pinned(sw, f"{name} {what}")
        if not c.zero_delta:
            mn.check_stops(c, sw)
    assert c.redrawn == 0.0


@pytest.mark.parametrize("w_min", mn.W_MINS)
@pytest.mark.parametrize("mode", ["fp32", "h2", "f16"])
@pytest.mark.parametrize("name", FUSED)
def test_fused_cases_are_pinned(name, mode, w_min):
    c, ref = _fused(name, mode, 40, w_min)
    assert c.redrawn <= sn.REDRAW_CAP
    mn.check_pinned(ref.sw, name)
    mn.check_stops(c, ref.sw)
    f = ref.f
    for a, e in ((f.a1, f.e_a1), (f.a2, f.e_a2), (f.a1s, f.e_a1s)):
        assert not sn._near_zero(a, e).any()


def test_fused_layout_case_reaches_its_mechanisms():
    c, ref = _fused("layouts")
    assert mn.rays_per_wave(c.n_cap) == 2
    cnt, keep = c.span[:c.n_alive, 1], ref.sw.keep.sum(1)
    pairs = list(zip(cnt[0::2], cnt[1::2]))
    assert (0, 9) in pairs and (9, 0) in pairs and (0, 0) in pairs           # empty first / last / all
    assert (c.span[7, 0] - c.span[6, 0]) % 64 == 0 and cnt[7] > 0            # a head at lane 0 of a chunk
    assert cnt[8] > 64 and cnt[10] > 128                                     # cut by one and by two boundaries
    assert keep[12] == 0 and keep[13] == 0 and cnt[12] > 0                   # a wave with no kept sample
    assert keep[14] > 128 and keep[10] == cnt[10]                            # the list drains in mid-ray
    assert c.n_alive < c.n_cap
    for n_cap, rpw in ((1, 2), (6144, 2), (6145, 3), (393216, 128), (393217, 128)):
        assert mn.rays_per_wave(n_cap) == rpw
    assert -(-393217 // (256 * mn.CMP_WAVES)) == 129


@pytest.mark.parametrize("name", MARCH)
def test_march_train_cases_are_pinned(name):
    c, fw, w32, t32, bw = _march(name)
    assert c.redrawn <= sn.REDRAW_CAP
    mn.check_pinned(fw.sw, name)
    if name == "span1025":
        # the over-long span is dropped like one that reaches M: zero outputs,
        # zero rows, and the spans after it in the stream are composited
        idx, off, cnt = c.rays[1]
        assert cnt == 1025 and fw.weights_sum[idx] == 0 and (fw.image[idx] == 0).all()
        assert (fw.w_out[off:off + cnt] == 0).all() and (bw.d_h[off:off + cnt] == 0).all()
        assert fw.weights_sum[c.rays[3, 0]] > 0 and fw.weights_sum[c.rays[2, 0]] > 0
    if name == "span1024":
        assert fw.sw.keep[1].sum() > 1000


# ---------------------------------------------------------------------------
# every mutant is rejected by a named case
# ---------------------------------------------------------------------------
# mutant -> (family, case): the GPU test runs the same case against the kernels
# of that family (train = ucsa_composite_rays_train_*, segment =
# ucsa_march_segment_composite, steps = ucsa_composite_rays, fused =
# ucsa_march_segment_shade*, march = ucsa_march_train_*), so the same mistake
# in a kernel fails there
KILLED_BY = {
    "stop_before_take": [("segment", "stop63"), ("steps", "stop64"), ("fused", "stops")],
    "never_stop": [("segment", "stop62"), ("steps", "stop128"), ("fused", "stops")],
    "carry_lost_64": [("train", "len65"), ("segment", "len129"), ("steps", "len65"),
                      ("fused", "layouts"), ("march", "small")],
    "t_from_zero": [("segment", "len2"), ("steps", "len1"), ("fused", "two"), ("march", "small")],
    "depth_unmasked": [("fused", "layouts"), ("march", "small")],
    "ws_masked": [("fused", "layouts"), ("march", "small")],
    "keep_span_ending_at_M": [("train", "dropped"), ("march", "dropped_last")],
    "sem_attached": [("train", "sem64"), ("march", "small")],
    "alpha_from_delta1": [("train", "len63"), ("segment", "len64"), ("steps", "len2"),
                          ("fused", "two"), ("march", "small")],
    "scale_ignored": [("segment", "scale"), ("fused", "two"), ("march", "small")],
    "finished_ignores_cap": [("segment", "cap_above"), ("fused", "cap_above")],
    "overwrite_not_add": [("segment", "len1"), ("steps", "len1"), ("fused", "single")],
    "suffix_inclusive": [("train", "len2"), ("march", "small")],
    "depth_grad_dropped": [("march", "small")],
    "keep_span_1025": [("march", "span1025")],
}


def _mutant_survives(family, case, mutant):
    m = (mutant,)
    if family == "train":
        c, fw, bw = _train(case)
        f2, b2 = mn.train_refs(c, mutant=m)
        return (mn.passes(mn.as_got(f2, mn.TRAIN_KEYS), fw, mn.TRAIN_KEYS)
                and mn.passes(mn.as_got(b2, mn.TRAIN_BWD_KEYS), bw, mn.TRAIN_BWD_KEYS))
    if family in ("segment", "steps"):
        c, seg, stp = _update(case)
        if family == "segment":
            got, ref = mn.segment_composite(*mn.update_args(c), mutant=m), seg
        else:
            got, ref = mn.composite_rays_update(*mn.steps_args(c), mutant=m), stp
        return mn.passes(mn.as_got(got, mn.UPDATE_KEYS), ref, mn.UPDATE_KEYS)
    if family == "fused":
        c, ref = _fused(case)
        got = mn.segment_shade(*mn.fused_args(c), mutant=m)
        return mn.passes(mn.as_got(got, mn.FUSED_KEYS), ref, mn.FUSED_KEYS)
    c, fw, w32, t32, bw = _march(case)
    f2 = mn.march_train_forward(*mn.march_fwd_args(c), mutant=m)
    b2 = mn.march_train_backward(*mn.march_bwd_args(c, w32, t32), mutant=m)
    return (mn.passes(mn.as_got(f2, mn.MARCH_FWD_KEYS), fw, mn.MARCH_FWD_KEYS)
            and mn.passes(mn.as_got(b2, mn.MARCH_BWD_KEYS), bw, mn.MARCH_BWD_KEYS))


def test_killed_by_names_every_mutant():
    assert set(KILLED_BY) == set(mn.MUTANTS)


@pytest.mark.parametrize("mutant,family,case",
                         [(m, f, c) for m, lst in KILLED_BY.items() for f, c in lst])
def test_mutant_is_rejected(mutant, family, case):
    assert not _mutant_survives(family, case, mutant), f"{mutant} passes {family}:{case}"


def test_clean_reference_passes_itself():
    """the predicate of the mutant table accepts the unmutated reference"""
    for family, case in (("train", "len65"), ("segment", "stop63"), ("steps", "stop64"),
                         ("fused", "layouts"), ("march", "small")):
        assert _mutant_survives(family, case, "none")


# ---------------------------------------------------------------------------
# the marched training reference against torch autograd
# ---------------------------------------------------------------------------
class _FieldOnRows:
    """the oracle field with its density replaced by given h rows (a leaf)"""

    def __init__(self, fld, h):
        from oracle.field import trunc_exp
        self.fld, self.h, self.C, self._exp = fld, h, fld.C, trunc_exp

    def density(self, x):
        return {"sigma": self._exp(self.h[:, 0]), "geo_feat": self.h[:, 1:]}

    def color(self, *a, **kw):
        return self.fld.color(*a, **kw)

    def semantics(self, *a, **kw):
        return self.fld.semantics(*a, **kw)


@pytest.mark.parametrize("w_min", [1e-4, 0.0])
def test_march_training_reference_matches_autograd(w_min):
    from tests.test_gpu_raymarch import _oracle_marched_render
    C = 17
    fld = lively_oracle_field(C=C).requires_grad_(True)
    cp, sp = fld.color_params.detach().numpy(), fld.sem_params.detach().numpy()
    c = mn.case_march_train("autograd", [5, 0, 70, 9, 3], C, w_min, cp, sp, seed=7, sigma_scale=1.0)
    h = torch.from_numpy(c.h.copy()).requires_grad_(True)
    sig = torch.exp(h[:, 0]).detach().numpy()          # the sigmas the torch pass composites
    xyz = np.zeros((c.M, 3), F32)
    out = _oracle_marched_render(_FieldOnRows(fld, h), np.zeros((c.N, 3), F32), c.rays_d, c.norms, c.nears,
                                 xyz, c.deltas, c.rays, w_min)
    img, dep, sem, wsum = out
    ((img * torch.from_numpy(c.d_image)).sum() + (dep * torch.from_numpy(c.d_depth)).sum()
     + (sem * torch.from_numpy(c.d_sem)).sum()).backward()
    args = list(mn.march_fwd_args(c))
    args[4] = sig
    fw = mn.march_train_forward(*args)
    mn.check_pinned(fw.sw, "autograd")
    got = dict(weights_sum=wsum.detach().numpy(), image=img.detach().numpy(), semantics=sem.detach().numpy(),
               depth=dep.detach().numpy() * c.norms)
    e_depth = fw.e_depth
    fw.e_depth = e_depth + 2.0 * sn.U * np.abs(fw.depth)        # the division and this product
    mn.compare_fields(got, fw, ("weights_sum", "depth", "image", "semantics"), "autograd fwd")
    w32, t32 = fw.w_out.astype(F32), fw.t_out.astype(F32)
    bargs = list(mn.march_bwd_args(c, w32, t32))
    bargs[4] = sig
    bw = mn.march_train_backward(*bargs)
    got = dict(d_h=h.grad.numpy(), dW_color=fld.color_params.grad.numpy(), dW_sem=fld.sem_params.grad.numpy())
    mn.compare_fields(got, bw, ("d_h", "dW_color", "dW_sem"), "autograd bwd")
