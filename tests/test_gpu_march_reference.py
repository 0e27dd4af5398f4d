"""The marched compositing entry points against the float64 reference of
tests/march_numpy.py, element by element, within bounds derived there from
counting rounding steps: ``ucsa_composite_rays_train_fwd/bwd``,
``ucsa_composite_rays``, ``ucsa_march_segment_composite``,
``ucsa_march_segment_shade{,_f16,_h2}`` and ``ucsa_march_train_fwd/bwd``.  The
spans are synthetic (no marcher, no hash grid): span lengths, stop positions,
slot layouts and class counts are placed by the case builders, every stop and
mask decision is pinned clear of its threshold, so there are no exempt samples
and no flat tolerance.  tests/test_march_reference_cpu.py holds the reference
against the C oracle and torch autograd and names, per deliberate mistake, the
case here that rejects it (``KILLED_BY``).

Worst err / bound per entry point and case family, as printed at the end of a
run on an MI355X: docs/DESIGN_NOTEBOOK.md, section MR."""
import functools

import numpy as np
import pytest
import torch

from tests import march_numpy as mn
from tests import shade_numpy as sn
from tests.util import lively_oracle_field

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    yield _ops
    if sn.WORST:
        print("\nworst err / bound per entry point, case family and output:")
        for k in sorted(sn.WORST):
            print(f"  {k}: {sn.WORST[k]:.3f}")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    """a faulted device ends the module: no later test launches on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _lib():
    from ucsa_neural_rendering_amd import _lib as L
    return L


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _i32(a):
    return _dev(np.asarray(a, np.int32), torch.int32)


class _Args:
    """pointers for a C ABI call; the device copies they point to stay alive
    until the caller has synchronised"""

    def __init__(self, ops):
        self.ptr, self.keep = ops._ptr, []

    def __call__(self, a, dtype=torch.float32):
        t = a if (a is None or torch.is_tensor(a)) else _dev(a, dtype)
        self.keep.append(t)
        return self.ptr(t)


def _bits(t):
    return np.atleast_1d(t.detach().cpu().contiguous().numpy()).view(np.uint8).tobytes()


def _family(name):
    return name.rstrip("0123456789")


@functools.lru_cache(maxsize=None)
def _params(C):
    fld = lively_oracle_field(C=C)
    return fld.color_params.numpy(), fld.sem_params.numpy()


# ---------------------------------------------------------------------------
# ucsa_composite_rays_train_fwd / _bwd
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train(name):
    c = mn.build_train_case(name)
    return (c,) + mn.train_refs(c)


def _run_train(ops, c):
    sig, rgb, ls, dl, rays = _dev(c.sigmas), _dev(c.rgbs), _dev(c.local_sem), _dev(c.deltas), _i32(c.rays)
    ws, depth, image, sem = ops.composite_rays_train_fwd(sig, rgb, ls, dl, rays)
    g = ops.composite_rays_train_bwd(_dev(c.g_ws), _dev(c.g_img), _dev(c.g_sem), sig, rgb, dl, rays, ws, image)
    torch.cuda.synchronize()
    return (dict(weights_sum=ws, depth=depth, image=image, semantics=sem),
            dict(grad_sigmas=g[0], grad_rgbs=g[1], grad_local_sem=g[2]))


@pytest.mark.parametrize("name", list(mn.train_case_specs()))
def test_composite_rays_train(ops, name):
    """forward sums by ray id and per-sample gradients (the backward is fed the
    kernel's own forward outputs, as autograd feeds it); dropped and empty spans
    give exact zeros in both (their bound is 0); a second call gives the same bits"""
    c, fw, bw = _train(name)
    got_f, got_b = _run_train(ops, c)
    fam = _family(name)
    mn.compare_fields(got_f, fw, mn.TRAIN_KEYS, f"composite_rays_train_fwd {fam}", name)
    mn.compare_fields(got_b, bw, mn.TRAIN_BWD_KEYS, f"composite_rays_train_bwd {fam}", name)
    again_f, again_b = _run_train(ops, c)
    for a, b in ((got_f, again_f), (got_b, again_b)):
        for k in a:
            assert a[k] is None or _bits(a[k]) == _bits(b[k]), f"{k}: second call differs"


def test_more_than_256_classes_is_an_argument_error_and_writes_nothing(ops):
    L = _lib()
    lib, p = L.lib(), _Args(ops)
    c = mn.case_train("sem257", [5, 70], 257, seed=1)
    sig, rgb, ls, dl, rays = _dev(c.sigmas), _dev(c.rgbs), _dev(c.local_sem), _dev(c.deltas), _i32(c.rays)
    fill = lambda *s: torch.full(s, 7.25, device="cuda")
    ws, depth, image, sem = fill(c.N), fill(c.N), fill(c.N, 3), fill(c.N, 257)
    gs, gr, gl = fill(c.M), fill(c.M, 3), fill(c.M, 257)
    rays_t, span = fill(c.N), _i32(c.rays[:, 1:])
    calls = (
        ("ucsa_composite_rays_train_fwd", 7, lambda: lib.ucsa_composite_rays_train_fwd(
            p(sig), p(rgb), p(ls), p(dl), p(rays), c.M, c.N, 257, p(ws), p(depth), p(image), p(sem), ops._stream())),
        ("ucsa_composite_rays_train_bwd", 11, lambda: lib.ucsa_composite_rays_train_bwd(
            p(c.g_ws), p(c.g_img), p(c.g_sem), p(sig), p(rgb), p(dl), p(rays), p(ws), p(image),
            c.M, c.N, 257, p(gs), p(gr), p(gl), ops._stream())),
        ("ucsa_march_segment_composite", 11, lambda: lib.ucsa_march_segment_composite(
            c.N, None, 70, p(rays), p(rays_t), p(span), p(sig), 1.0, p(rgb), p(ls), p(dl), 257, p(ws), p(depth),
            p(image), p(sem), ops._stream())),
    )
    for what, arg, call in calls:
        rc = call()
        assert rc == -1000 - arg, (what, rc)              # UCSA_ERR_ARG - k
        with pytest.raises(L.UcsaError, match=f"code {-1000 - arg}"):
            L.check(rc, what)
    torch.cuda.synchronize()
    for t in (ws, depth, image, sem, gs, gr, gl, rays_t):
        assert bool((t == 7.25).all())


# ---------------------------------------------------------------------------
# ucsa_march_segment_composite and ucsa_composite_rays
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _update(name):
    c = mn.build_update_case(name)
    return c, mn.segment_composite(*mn.update_args(c)), mn.composite_rays_update(*mn.steps_args(c))


def _state(c):
    return dict(rays_t=_dev(c.rays_t), weights_sum=_dev(c.weights_sum), depth=_dev(c.depth),
                image=_dev(c.image), semantics=_dev(c.semantics))


def _run_segment(ops, c, slots=None):
    """``ucsa_march_segment_composite`` on the case (n_alive on the device), or
    on the given slots alone (n_alive_dev = NULL)"""
    L = _lib()
    p = _Args(ops)
    st = _state(c)
    if slots is None:
        n_cap, n_dev = c.n_cap, _i32([c.n_alive])
        ra, rt, span = _i32(c.rays_alive), st["rays_t"], _i32(c.span)
    else:
        n_cap, n_dev = len(slots), None
        ra, span = _i32(c.rays_alive[slots]), _i32(c.span[slots])
        rt = st["rays_t"] = _dev(c.rays_t[slots])
    L.check(L.lib().ucsa_march_segment_composite(
        n_cap, p(n_dev), c.cap, p(ra), p(rt), p(span), p(c.sigmas), float(c.sigma_scale), p(c.rgbs),
        p(c.local_sem), p(c.deltas), c.n_sem, p(st["weights_sum"]), p(st["depth"]), p(st["image"]),
        p(st["semantics"]), ops._stream()), "ucsa_march_segment_composite")
    torch.cuda.synchronize()
    return st


def _run_steps(ops, c):
    n_alive, n_step, ra, _, sig, rgb, ls, dl = mn.steps_args(c)[:8]
    st = _state(c)
    ops.composite_rays(n_alive, n_step, _i32(ra), st["rays_t"], _dev(sig), _dev(rgb), _dev(ls), _dev(dl),
                       st["weights_sum"], st["depth"], st["image"], st["semantics"])
    torch.cuda.synchronize()
    return st


def _check_update(c, got, ref, what, name):
    mn.compare_fields(got, ref, mn.UPDATE_KEYS, what, name)
    rt = got["rays_t"].cpu().numpy()
    assert ((rt[:c.n_alive] == -1) == ref.finished).all(), "finished rays"
    # what the contract leaves alone, as bytes: slots past the alive count and
    # every ray that is no alive slot's
    assert rt[c.n_alive:].tobytes() == c.rays_t[c.n_alive:].tobytes()
    idle = np.setdiff1d(np.arange(c.N), c.rays_alive[:c.n_alive])
    assert idle.size >= 2
    for k in ("weights_sum", "depth", "image", "semantics"):
        if got[k] is not None:
            assert got[k].cpu().numpy()[idle].tobytes() == getattr(c, k)[idle].tobytes(), k


@pytest.mark.parametrize("name", list(mn.update_case_specs()))
def test_segment_composite(ops, name):
    c, ref, _ = _update(name)
    got = _run_segment(ops, c)
    _check_update(c, got, ref, f"march_segment_composite {_family(name)}", name)
    again = _run_segment(ops, c)
    assert all(got[k] is None or _bits(got[k]) == _bits(again[k]) for k in got), "second call differs"
    # a slot computed alone gives the bits it gives inside the batch
    for s in {0, c.n_alive - 1}:
        alone = _run_segment(ops, c, [s])
        ray = int(c.rays_alive[s])
        assert _bits(alone["rays_t"][0]) == _bits(got["rays_t"][s])
        for k in ("weights_sum", "depth", "image", "semantics"):
            assert got[k] is None or _bits(alone[k][ray]) == _bits(got[k][ray]), (k, s)


@pytest.mark.parametrize("name", list(mn.update_case_specs()))
def test_composite_rays(ops, name):
    """the padded-row form of the same slots (a zero delta0 ends a ray)"""
    c, _, ref = _update(name)
    got = _run_steps(ops, c)
    _check_update(c, got, ref, f"composite_rays {_family(name)}", name)
    again = _run_steps(ops, c)
    assert all(got[k] is None or _bits(got[k]) == _bits(again[k]) for k in got), "second call differs"


# ---------------------------------------------------------------------------
# ucsa_march_segment_shade, _f16, _h2
# ---------------------------------------------------------------------------
MODES = {"fp32": sn.FP32, "f16": sn.F16M(1024.0), "h2": sn.H2}
ENTRY = {"march_segment_shade": "fp32", "march_segment_shade_f16": "f16", "march_segment_shade_h2": "h2"}


@functools.lru_cache(maxsize=None)
def _fused(name, mode, C, w_min):
    if name.startswith("wide"):
        n_cap = int(name[4:])
        wide = n_cap > 100000        # spans of 0 or 1 samples, few of them: the reference stays small
        c = mn.case_fused_wide(n_cap, *_params(C), MODES[mode], C=C, w_min=w_min,
                               max_count=1 if wide else 2, fill=0.03 if wide else 0.5)
    else:
        c = mn.build_fused_case(name, *_params(C), MODES[mode], C=C, w_min=w_min)
    return c, mn.segment_shade(*mn.fused_args(c))


def _packs(ops, c, mode):
    L = _lib()
    cp, sp = _dev(c.color_params), _dev(c.sem_params)
    pack = {"fp32": ops.mlp_pack, "f16": ops.mlp_pack_f16, "h2": ops.mlp_pack_h2}[mode]
    return pack(L.MLP_COLOR, cp, c.C), pack(L.MLP_SEM, sp, c.C)


def _run_fused(ops, c, mode, slots=None, n_dev="tensor"):
    L = _lib()
    p = _Args(ops)
    fn = getattr(L.lib(), {"fp32": "ucsa_march_segment_shade", "f16": "ucsa_march_segment_shade_f16",
                           "h2": "ucsa_march_segment_shade_h2"}[mode])
    st = _state(c)
    if slots is None:
        n_cap = c.n_cap
        nd = _i32([c.n_alive]) if n_dev == "tensor" else None
        ra, rt, span = _i32(c.rays_alive), st["rays_t"], _i32(c.span)
    else:
        n_cap, nd = len(slots), None
        ra, span = _i32(c.rays_alive[slots]), _i32(c.span[slots])
        rt = st["rays_t"] = _dev(c.rays_t[slots])
    pc, ps = _packs(ops, c, mode)
    L.check(fn(n_cap, p(nd), c.cap, p(ra), p(rt), p(span), p(c.rays_d), p(c.sigmas),
               float(c.sigma_scale), p(c.h), p(c.deltas), p(pc), p(ps), c.C, float(c.w_min),
               p(st["weights_sum"]), p(st["depth"]), p(st["image"]), p(st["semantics"]), ops._stream()),
            "ucsa_march_segment_shade")
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("w_min", mn.W_MINS)
@pytest.mark.parametrize("name", list(mn.fused_case_specs()))
@pytest.mark.parametrize("entry", list(ENTRY))
def test_segment_shade(ops, entry, name, w_min):
    mode = ENTRY[entry]
    c, ref = _fused(name, mode, 40, w_min)
    got = _run_fused(ops, c, mode)
    _check_update(c, got, ref, f"{entry} {name}", f"w_min={w_min:g}")
    again = _run_fused(ops, c, mode)
    assert all(_bits(got[k]) == _bits(again[k]) for k in got), "second call differs"
    # the first slot of a wave, computed alone, gives the bits it gives in the batch
    s = 2 * ((c.n_alive - 1) // 2)
    alone = _run_fused(ops, c, mode, [s])
    ray = int(c.rays_alive[s])
    assert _bits(alone["rays_t"][0]) == _bits(got["rays_t"][s])
    for k in ("weights_sum", "depth", "image", "semantics"):
        assert _bits(alone[k][ray]) == _bits(got[k][ray]), (k, s)


@pytest.mark.parametrize("C", [v for v in mn.CLASS_COUNTS if v != 40])
@pytest.mark.parametrize("entry", list(ENTRY))
def test_segment_shade_class_counts(ops, entry, C):
    mode = ENTRY[entry]
    c, ref = _fused("layouts", mode, C, 1e-4)
    _check_update(c, _run_fused(ops, c, mode), ref, f"{entry} classes", f"C={C}")


@pytest.mark.parametrize("n_cap", [6145, 393217])
@pytest.mark.parametrize("entry", list(ENTRY))
def test_segment_shade_many_slots(ops, entry, n_cap):
    """three slots per wave (empty ones in the middle of a wave's range), and the
    clamp of the slots per wave to the LDS tables' 128; n_alive_dev = NULL"""
    mode = ENTRY[entry]
    assert mn.rays_per_wave(n_cap) == (3 if n_cap == 6145 else mn.RPW_MAX)
    c, ref = _fused(f"wide{n_cap}", mode, 40, 1e-4)
    assert c.n_alive == c.n_cap
    got = _run_fused(ops, c, mode, n_dev=None)
    mn.compare_fields(got, ref, mn.FUSED_KEYS, f"{entry} wide", f"n_cap={n_cap}")
    assert ((got["rays_t"].cpu().numpy() == -1) == ref.finished).all()


@pytest.mark.parametrize("name", ["layouts", "stops"])
def test_fused_and_unfused_agree_at_w_min_0(ops, name):
    """w_min = 0: the fused kernel and ucsa_point_shade_h +
    ucsa_march_segment_composite compute the same sums, each within its bound of
    the reference, so within the sum of the two of each other"""
    L = _lib()
    c, ref = _fused(name, "fp32", 40, 0.0)
    fused = _run_fused(ops, c, "fp32")
    pc, ps = _packs(ops, c, "fp32")
    rgb, probs = ops.point_shade_h(_dev(c.rays_d[c.sample_ray]), _dev(c.h), pc, ps, c.C)
    u = mn.NS(**vars(c))
    u.rgbs, u.local_sem, u.n_sem = rgb.cpu().numpy(), probs.cpu().numpy(), c.C
    unfused = _run_segment(ops, u)
    other = mn.segment_shade(sn.X3, *mn.fused_args(c)[1:])        # a bound for the point_shade nets
    for k in mn.FUSED_KEYS:
        a, b = fused[k].cpu().numpy().astype(F64), unfused[k].cpu().numpy().astype(F64)
        bound = getattr(ref, "e_" + k) + getattr(other, "e_" + k)
        sn.compare(a, b, bound, f"fused vs unfused {k} @ {name}")
    assert ((fused["rays_t"] == -1) == (unfused["rays_t"] == -1)).all()


# ---------------------------------------------------------------------------
# ucsa_march_train_fwd / _bwd
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march(name, C, w_min):
    c = mn.build_march_train_case(name, *_params(C), C=C, w_min=w_min)
    fw = mn.march_train_forward(*mn.march_fwd_args(c))
    w32, t32 = fw.w_out.astype(F32), fw.t_out.astype(F32)
    return c, fw, w32, t32, mn.march_train_backward(*mn.march_bwd_args(c, w32, t32))


def _run_march(ops, c, w32, t32):
    L = _lib()
    lib, p = L.lib(), _Args(ops)
    cp, sp = _dev(c.color_params), _dev(c.sem_params)
    pc, ps = ops.mlp_pack(L.MLP_COLOR, cp, c.C), ops.mlp_pack(L.MLP_SEM, sp, c.C)
    pct, pst = ops.mlp_pack_t(L.MLP_COLOR, cp, c.C), ops.mlp_pack_t(L.MLP_SEM, sp, c.C)
    rays, rays_d, sig, h, dl = _i32(c.rays), _dev(c.rays_d), _dev(c.sigmas), _dev(c.h), _dev(c.deltas)
    ws, depth, image, sem, w, t = ops.march_train_fwd(rays, c.M, _dev(c.nears), rays_d, sig, c.sigma_scale, h, dl,
                                                      pc, ps, c.C, c.w_min)
    fwd = dict(weights_sum=ws, depth=depth, image=image, semantics=sem, w_out=w, t_out=t)
    # the backward on the reference's fp32 weights, every output NaN before the call
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    parts = int(lib.ucsa_composite_bwd_parts(c.N))
    nrb = (c.C + 15) // 16
    G, d_h, ppc, pps = nan(c.M), nan(c.M, 16), nan(parts, 7168), nan(parts, 1024 + 1024 * nrb)
    L.check(lib.ucsa_march_train_bwd(
        p(rays), c.N, c.M, p(rays_d), p(c.norms), p(sig), float(c.sigma_scale), p(h), p(dl), p(w32),
        p(t32), p(pc), p(ps), p(pct), p(pst), c.C, float(c.w_min), p(c.d_image), p(c.d_depth),
        p(c.d_sem), p(G), p(d_h), p(ppc), p(pps), ops._stream()), "ucsa_march_train_bwd")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ppc).all()) and bool(torch.isfinite(pps).all()), "a wave left its partials unwritten"
    gc, gsem = torch.empty(7168, device="cuda"), torch.empty(pps.shape[1], device="cuda")
    ops.reduce_partials(ppc, gc, False)
    ops.reduce_partials(pps, gsem, False)
    torch.cuda.synchronize()
    return fwd, dict(G=G, d_h=d_h, dW_color=gc, dW_sem=gsem)


def _check_march(ops, name, C, w_min, what):
    c, fw, w32, t32, bw = _march(name, C, w_min)
    fwd, bwd = _run_march(ops, c, w32, t32)
    mn.compare_fields(fwd, fw, mn.MARCH_FWD_KEYS, f"march_train_fwd {what}", f"{name} C={C} w_min={w_min:g}")
    # G is scratch outside the composited spans (NaN as given); inside, every row
    G = bwd["G"].cpu().numpy()
    assert np.isnan(G[~bw.composited]).all()
    bwd["G"] = np.where(bw.composited, G, 0.0)
    mn.compare_fields(bwd, bw, mn.MARCH_BWD_KEYS, f"march_train_bwd {what}", f"{name} C={C} w_min={w_min:g}")
    return c, fw, bw, fwd, bwd


@pytest.mark.parametrize("w_min", mn.W_MINS)
@pytest.mark.parametrize("name", ["small", "span1024", "dropped_last"])
def test_march_train(ops, name, w_min):
    """per-ray sums, per-sample w / t, and per-sample G and d_h, dW of both nets"""
    _check_march(ops, name, 40, w_min, name)


@pytest.mark.parametrize("C", [v for v in mn.CLASS_COUNTS if v != 40])
def test_march_train_class_counts(ops, C):
    _check_march(ops, "small", C, 1e-4, "classes")


def test_march_train_drops_a_span_longer_than_1024(ops):
    """include/ucsa_hip.h: a rays row with count > 1024 is dropped by both passes
    like one that reaches M -- zero outputs, zero w / t / d_h rows, G untouched --
    and the spans after it in the stream are composited as usual"""
    c, fw, bw, fwd, bwd = _check_march(ops, "span1025", 40, 1e-4, "span1025")
    idx, off, cnt = (int(v) for v in c.rays[1])
    assert cnt == 1025
    assert float(fwd["weights_sum"][idx]) == 0 and not bool(fwd["image"][idx].any())
    assert not bool(fwd["w_out"][off:off + cnt].any()) and not bool(bwd["d_h"][off:off + cnt].any())
    assert float(fwd["weights_sum"][int(c.rays[3, 0])]) > 0
