"""The density reference (tests/density_numpy.py, ``shade_numpy.sigma_forward``
with ``outputs=True``) held against the oracle and against itself, on the CPU:

* its float64 values are ``oracle.field.mlp_forward`` + ``exp`` in float64;
* plain fp32 with sequential sums, the oracle's fp32 path and its
  ``emulate_fp16`` path stay inside the corresponding bounds on every case
  family (the bounds are not tighter than correct arithmetic needs), worst
  err / bound recorded in ``WORST_CPU``;
* ``density_rays`` agrees with the oracle's encoder + sigma net;
* every deliberate mistake of ``density_numpy.MUTANTS`` is rejected by the SAME
  ``compare_density`` call the GPU tests make, on the smallest case named in
  ``KILLED_BY``;
* the sigma interval at the overflow straddle, at the subnormal edge and at the
  exact zero, by hand.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import field as ofield
from oracle.fixtures import lively_oracle_field
from tests import density_numpy as dn
from tests import hashgrid_numpy as hn
from tests import shade_numpy as sn

F32, F64 = np.float32, np.float64
WORST_CPU = {}


@functools.lru_cache(maxsize=None)
def field():
    return lively_oracle_field()


@functools.lru_cache(maxsize=None)
def weights(name):
    return field().sigma_params.numpy() if name == "w0" else dn.scaled_weights()


@functools.lru_cache(maxsize=None)
def rows_case(family, key, wname):
    if family == "sizes":
        return dn.case_sizes(key)
    if family == "magnitudes":
        return dn.case_magnitudes(f16=bool(key))
    return dn.case_exp(weights(wname))


@functools.lru_cache(maxsize=None)
def rows_ref(family, key, wname, mode):
    return dn.density_rows(rows_case(family, key, wname).x, weights(wname), mode)


ROW_CASES = [("sizes", M, "w0") for M in (1, 15, 17, 65, 257)] + \
            [("sizes", 129, "w8"), ("magnitudes", 0, "w0"), ("magnitudes", 0, "w8"),
             ("magnitudes", 1, "w0"), ("exp", None, "w0"), ("exp", None, "w8")]
row_id = lambda c: f"{c[0]}{'' if c[1] is None else c[1]}-{c[2]}"


def note(key, worst):
    WORST_CPU[key] = max(WORST_CPU.get(key, 0.0), worst)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST_CPU:
        print("\nworst err / bound of correct evaluations per case family:")
        for k in sorted(WORST_CPU):
            print(f"  {k}: {WORST_CPU[k]:.3f}")


def oracle_rows(x, w, emulate_fp16=False, double=False):
    spec = field().sigma_spec
    dt = torch.float64 if double else torch.float32
    h = ofield.mlp_forward(spec, torch.from_numpy(np.asarray(x, F32)).to(dt),
                           torch.from_numpy(np.asarray(w, F32)).to(dt), emulate_fp16)
    return h, torch.exp(h[:, 0])


# ---------------------------------------------------------------------------
# the reference is the oracle's net
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ROW_CASES if c[:2] != ("magnitudes", 1)], ids=row_id)
def test_float64_values_are_the_oracles(case):
    """to 2^-20 of each element's fp32 bound (both are float64 sums of the same
    terms in different orders); the fp16-only rows belong to the fp16 reference"""
    c, ref = rows_case(*case), rows_ref(*case, "fp32")
    h, sigma = oracle_rows(c.x, weights(case[2]), double=True)
    assert sn.worst_ratio(np.abs(h.numpy() - ref.h), ref.e_h * 2.0 ** -20) <= 1.0
    with np.errstate(over="ignore"):
        mid = np.exp(ref.h[:, 0])
    fin = np.isfinite(mid)                              # (float64 itself overflows beyond h0 = 709)
    sigma = sigma.numpy()
    assert np.array_equal(sigma[~fin], mid[~fin])
    width = (ref.sigma_hi[fin] - ref.sigma_lo[fin]) * 2.0 ** -20
    assert sn.worst_ratio(np.abs(sigma[fin] - mid[fin]), width) <= 1.0
    assert ((ref.sigma_lo <= mid) & (mid <= ref.sigma_hi)).all()


@pytest.mark.parametrize("case", ROW_CASES, ids=row_id)
def test_correct_evaluations_stay_inside_the_bounds(case):
    c, w = rows_case(*case), weights(case[2])
    fam = case[0]
    f16_only = case[:2] == ("magnitudes", 1)
    if not f16_only:
        for mode in ("fp32", "x3", "h2"):
            # plain fp32, sequential sums: fp32 arithmetic itself fits every fp32-grade bound
            h, s = dn.evaluate(c.x, w, "fp32", dt=F32)
            note(f"plain fp32 vs {mode} {fam}",
                 dn.compare_density(h, s, rows_ref(*case, mode), f"plain-fp32/{mode} {fam} @ {c.name}"))
        h, s = oracle_rows(c.x, w)
        note(f"oracle fp32 {fam}", dn.compare_density(h, s, rows_ref(*case, "fp32"),
                                                      f"oracle-fp32 {fam} @ {c.name}"))
    if fam != "exp":
        h, s = oracle_rows(c.x, w, emulate_fp16=True)
        note(f"oracle emulate_fp16 {fam}", dn.compare_density(h, s, rows_ref(*case, "f16"),
                                                              f"oracle-f16 {fam} @ {c.name}"))
        h, s = dn.evaluate(c.x, w, "f16")
        note(f"float64 fp16-emulating {fam}", dn.compare_density(h, s, rows_ref(*case, "f16"),
                                                                 f"f64-f16 {fam} @ {c.name}"))


def test_zero_row_is_exact():
    c = rows_case("magnitudes", 0, "w0")
    for mode in dn.MODES:
        ref = rows_ref("magnitudes", 0, "w0", mode)
        assert (ref.h[c.zero_row] == 0).all() and (ref.e_h[c.zero_row] == 0).all()
        assert ref.sigma_lo[c.zero_row] == 1.0 == ref.sigma_hi[c.zero_row]


def test_overflow_row_is_not_finite_in_fp16_only():
    c = rows_case("magnitudes", 1, "w0")
    ref = rows_ref("magnitudes", 1, "w0", "f16")
    bad = ~np.isfinite(ref.h).all(1)
    assert bad[c.overflow_row] and bad.sum() == 1
    assert not np.isfinite(ref.h[c.overflow_row]).any()
    # every first-layer weight the inf meets is non-zero in fp16: no inf * 0
    assert (sn.q16(weights("w0")[:2048].reshape(64, 32)[:, 9]) != 0).all()


# ---------------------------------------------------------------------------
# the fused path: encoder + net
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused(H, W, T):
    fld = field()
    levels = hn.levels_of(fld.grid)
    c = dn.case_fused(H, W, T, fld.bound)
    c.levels, c.table = levels, fld.grid_params.numpy().reshape(-1, 2)
    c.aabb = hn.aabb_of(fld.bound)
    c.pts = hn.ray_points(c.o, c.d, c.z, c.aabb)
    return c


@functools.lru_cache(maxsize=None)
def fused_ref(H, W, T, mode):
    c = fused(H, W, T)
    return dn.density_rays(c.levels, field().bound, c.table, c.o, c.d, c.z, c.aabb,
                           weights("w0"), mode)


@pytest.mark.parametrize("shape", [(8, 8, 1), (9, 17, 5), (8, 8, 17)], ids=str)
def test_density_rays_matches_the_oracle(shape):
    fld, c = field(), fused(*shape)
    x01 = torch.from_numpy(hn.unit_coords(c.pts, fld.bound))
    enc = ofield.hashgrid_encode(fld.grid, x01, fld.grid_params)
    h = ofield.mlp_forward(fld.sigma_spec, enc, fld.sigma_params)
    for mode in ("fp32", "x3", "h2"):
        note(f"oracle encoder + net vs {mode} fused",
             dn.compare_density(h, torch.exp(h[:, 0]), fused_ref(*shape, mode),
                                f"oracle {mode} fused @ {c.name}"))
        # plain fp32 with sequential sums on the oracle's fp32 features
        hs, ss = dn.evaluate(enc.numpy(), weights("w0"), "fp32", dt=F32)
        note(f"plain fp32 vs {mode} fused",
             dn.compare_density(hs, ss, fused_ref(*shape, mode), f"plain-fp32/{mode} fused @ {c.name}"))
    # some rays miss the box, some samples sit on the far faces
    on_face = (np.abs(c.pts) == fld.bound).any(1).reshape(c.H * c.W, c.T)
    assert on_face.all(1).any() and on_face[::11, -1].all()


# ---------------------------------------------------------------------------
# sharpness: wrong implementations are rejected
# ---------------------------------------------------------------------------
# mutant -> (family, key, mode): the smallest case of the GPU module that rejects it
KILLED_BY = {
    "cols_c_major": [("sizes", 1, "fp32"), ("sizes", 1, "h2")],
    "w2_rows_swapped": [("sizes", 1, "fp32"), ("sizes", 1, "f16")],
    "sigma_from_h1": [("sizes", 1, "fp32")],
    "sigma_clamped": [("exp", None, "fp32"), ("exp", None, "h2")],
    "relu_dropped": [("sizes", 15, "fp32"), ("sizes", 15, "x3")],
    "f16_hidden_unrounded": [("sizes", 1, "f16")],
    "tail_block_last_row": [("sizes", 15, "fp32"), ("sizes", 63, "fp32")],
    "scatter_to_m": [("scatter", "random", "fp32"), ("scatter", "reverse", "h2")],
    "fused_level_12_for_8": [("fused", (8, 8, 1, 8), "x3")],
    "fused_no_tile_base": [("fused", (9, 17, 5, 8), "h2"), ("fused", (9, 17, 5, 12), "x3")],
    "fused_table_row_late": [("fused", (8, 8, 1, 8), "x3"), ("fused", (8, 8, 1, 12), "h2")],
}
SCATTER_M = 300


def _survives(mutant, family, key, mode):
    """True when ``compare_density`` accepts the mutant's output on the case."""
    w = weights("w0")
    try:
        if family == "fused":
            H, W, T, n_enc = key
            c, ref = fused(H, W, T), fused_ref(H, W, T, mode)
            x = dn.to_rows(ref.feat) if mutant == "none" else \
                dn.fused_mutant_rows(ref, c.levels, field().bound, c.table, c.pts, H, W, T, n_enc, mutant)
            h, s = dn.evaluate(x, w, "fp32")
            dn.compare_density(h, s, ref, f"{mutant} fused @ {c.name}")
        elif family == "scatter":
            c = dn.case_sizes(SCATTER_M)
            ref = dn.density_rows(c.x, w, mode)
            slot = dn.slots(SCATTER_M, key)
            h, s = dn.evaluate(c.x, w, mode)
            out_h, out_s = np.full_like(h, np.nan), np.full_like(s, np.nan)
            at = np.arange(SCATTER_M) if mutant == "scatter_to_m" else slot
            out_h[at], out_s[at] = h, s
            # row slot[m] of the outputs belongs to sample m
            dn.compare_density(out_h[slot], out_s[slot], ref, f"{mutant} scatter @ {key}")
        else:
            c = dn.case_sizes(key) if family == "sizes" else rows_case(family, key, "w0")
            ref = dn.density_rows(c.x, w, mode)
            h, s = dn.evaluate(c.x, w, mode, mutant)
            dn.compare_density(h, s, ref, f"{mutant} {family} @ {c.name}")
    except sn.Mismatch:
        return False
    return True


def test_mutant_table_is_complete():
    assert set(KILLED_BY) == set(dn.MUTANTS)


@pytest.mark.parametrize("mutant,family,key,mode",
                         [(m, *k) for m, lst in KILLED_BY.items() for k in lst], ids=str)
def test_mutant_is_rejected(mutant, family, key, mode):
    assert _survives("none", family, key, mode), "the clean evaluation must pass the same call"
    assert not _survives(mutant, family, key, mode), f"{mutant} passes {family}:{key}"


def test_what_the_cases_cannot_see():
    """the identity slot hides a scatter to m; one tile hides a lost tile base;
    16 levels inside hide everything about feat_ws; M = 17 hides a tail block
    that copies row M - 1 (its tail block IS row M - 1 alone)"""
    assert _survives("scatter_to_m", "scatter", "identity", "fp32")
    assert _survives("fused_no_tile_base", "fused", (8, 8, 17, 8), "x3")
    assert _survives("fused_table_row_late", "fused", (8, 8, 1, 16), "x3")
    assert _survives("fused_level_12_for_8", "fused", (8, 8, 1, 12), "x3")
    assert _survives("tail_block_last_row", "sizes", 17, "fp32")


# ---------------------------------------------------------------------------
# the sigma interval by hand
# ---------------------------------------------------------------------------
def test_sigma_interval_by_hand():
    ln_max = math.log(sn.FLT_MAX)                       # 88.7228...
    inf, big = np.float32(np.inf), np.float32(sn.FLT_MAX)
    # the straddle: h0 within e of ln FLT_MAX allows inf and a finite value
    lo, hi = sn.sigma_interval([ln_max], [1e-3])
    assert lo[0] < sn.FLT_MAX < hi[0]
    assert sn.in_sigma_interval([inf], lo, hi)[0] and sn.in_sigma_interval([big], lo, hi)[0]
    assert not sn.in_sigma_interval([np.float32(3.3e38)], lo, hi)[0]     # below exp(h0 - e)
    # beyond it inf is required, below it inf is refused
    lo, hi = sn.sigma_interval([89.0, 88.0], [1e-3, 1e-3])
    assert list(sn.in_sigma_interval([inf, inf], lo, hi)) == [True, False]
    assert list(sn.in_sigma_interval([big, np.float32(math.exp(88.0))], lo, hi)) == [False, True]
    # the subnormal edge: exp(-87.4) ~ 1.1e-38 < 2^-126: flushed to 0 or kept
    lo, hi = sn.sigma_interval([-87.4], [0.0])
    assert lo[0] == 0.0 and math.exp(-87.4) < hi[0] <= math.exp(-87.4) * 1.0001 + 2.0 ** -126
    assert sn.in_sigma_interval([np.float32(0.0)], lo, hi)[0]
    assert sn.in_sigma_interval([np.float32(math.exp(-87.4))], lo, hi)[0]
    assert not sn.in_sigma_interval([np.float32(3e-38)], lo, hi)[0]
    # just above it nothing is flushed: exp(-87.0) ~ 1.6e-38 is normal
    lo, hi = sn.sigma_interval([-87.0], [0.0])
    assert lo[0] > 0.0 and not sn.in_sigma_interval([np.float32(0.0)], lo, hi)[0]
    # -110: below the smallest subnormal, 0 and anything up to 2^-126 pass
    lo, hi = sn.sigma_interval([-110.0], [1e-4])
    assert lo[0] == 0.0 and sn.in_sigma_interval([np.float32(0.0)], lo, hi)[0]
    # the exact zero: 1.0 and nothing else; a zero value with a bound is an interval
    lo, hi = sn.sigma_interval([0.0, 0.0], [0.0, 1e-6])
    assert lo[0] == hi[0] == 1.0 and lo[1] < 1.0 < hi[1]
    assert list(sn.in_sigma_interval([np.float32(1.0), np.float32(1.0)], lo, hi)) == [True, True]
    assert not sn.in_sigma_interval([np.nextafter(np.float32(1.0), np.float32(2.0))], lo[:1], hi[:1])[0]
    # an overflowed h0 (fp16 features beyond 65504): inf and 0 whatever its bound holds
    lo, hi = sn.sigma_interval([np.inf, -np.inf], [np.nan, np.inf])
    assert list(sn.in_sigma_interval([inf, np.float32(0.0)], lo, hi)) == [True, True]
    assert list(sn.in_sigma_interval([big, np.float32(1.0)], lo, hi)) == [False, False]
    # NaN in, NaN out
    lo, hi = sn.sigma_interval([np.nan], [0.0])
    assert sn.in_sigma_interval([np.float32(np.nan)], lo, hi)[0]
    assert not sn.in_sigma_interval([np.float32(1.0)], lo, hi)[0]


def test_sigma_backward_is_unchanged():
    """``sigma_forward`` without ``outputs`` is what ``sigma_backward`` always read"""
    c = sn.build_sigma_case(weights("w0"), 65)
    f = sn.sigma_forward(c.feat, c.sigma_params, sn.X2, False)
    W1 = np.asarray(c.sigma_params, F64)[:2048].reshape(64, 32)
    a1, e_a1 = sn._lin(np.asarray(c.feat, F64), np.zeros(c.feat.shape), W1, sn.X2, F64)
    assert np.array_equal(f.a1, a1) and np.array_equal(f.e_a1, e_a1)
    assert not hasattr(f, "h")
