"""The float64 resampling reference of tests/resample_numpy.py, without a GPU:
it reproduces the oracle and the recorded ``sample_pdf`` samples within its own
intervals; plain fp32 evaluations in three summation orders stay inside them
on every case of the GPU test (the bounds are not tighter than fp32 allows);
every deliberate mistake that CAN show is rejected by a named case (the
intervals are not so wide that a wrong kernel would pass); and on the sharp
cases at most 5 % of the samples have more than one allowed interval."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import renderer as oren
from tests import resample_numpy as rn

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _case(name):
    c = rn.build_case(name)
    return c, rn.reference(c.z, c.sigma, c.u, c.density_scale)


# the shapes and inputs of tests/test_gpu_parity.py::test_resample_matches_oracle
@pytest.mark.parametrize("T,t", [(16, 16), (96, 96), (256, 256), (8, 40)])
def test_reference_reproduces_oracle(T, t):
    g = torch.Generator().manual_seed(T + t)
    N = 257
    z = torch.sort(torch.rand(N, T, generator=g) * 7 + 0.2, -1)[0]
    sigma = (torch.rand(N, T, generator=g) * 3).pow(3)
    sigma[0] = 0.0
    u = torch.rand(N, t, generator=g)
    u[1, 0] = 0.0
    deltas, w = oren.alpha_weights(z, sigma, 1.0)
    got = oren.inverse_cdf(z[:, :-1] + 0.5 * deltas[:, :-1], w[:, 1:-1], torch.sort(u, dim=-1)[0])
    ref = rn.reference(z, sigma, u, 1.0)
    rn.check(got, ref, f"oracle T={T} t={t}")
    # and stage by stage: the weights and the midpoints within their bounds
    assert (np.abs(w.numpy().astype(np.float64) - ref.rw.w) <= ref.rw.e_w).all()
    bins = (z[:, :-1] + 0.5 * deltas[:, :-1]).numpy().astype(np.float64)
    assert (np.abs(bins - ref.rw.bins) <= ref.rw.e_bins).all()


def test_inversion_reproduces_recorded_sample_pdf():
    """tests/golden/g3_sample_pdf.npz: the reference project's own sample_pdf
    (all-zero weights, flat cdf segments, weights of 1e-7, u = 0 and the last
    fp32 number below 1), in the order of u."""
    g = np.load(os.path.join(GOLDEN, "g3_sample_pdf.npz"))
    ref = rn.invert_reference(g["bins"], g["weights"], g["u"], sort=False)
    rn.check(g["samples"], ref, "recorded sample_pdf")
    # sorted, the same samples permuted
    order = np.argsort(g["u"], axis=1, kind="stable")
    ref = rn.invert_reference(g["bins"], g["weights"], g["u"], sort=True)
    rn.check(np.take_along_axis(g["samples"], order, 1), ref, "recorded sample_pdf, sorted")


def test_exact_steps_carry_no_bound():
    """where the source is exact the reference claims exactness: alpha of a
    zero optical depth, T_0, cdf_0, and the clamped ends of the inversion"""
    c, ref = _case("T64_t64_zero")
    rw = ref.rw
    assert (rw.alpha[:, :-1] == 0).all() and (rw.e_alpha[:, :-1] == 0).all()
    assert (rw.e_T[:, 0] == 0).all() and (ref.e_cdf[:, 0] == 0).all()
    assert (rw.e_w[:, :-1] == 0).all()
    c, ref = _case("T129_t128_zmax")
    assert (ref.value == c.z[:, :1]).all()
    assert (rn.ratios(c.z[:, :1].repeat(c.t, 1), ref) == 0).all()


@pytest.mark.parametrize("order", rn.ORDERS)
@pytest.mark.parametrize("name", rn.CASE_NAMES)
def test_fp32_evaluation_lies_inside(name, order):
    c, ref = _case(name)
    got = rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, order)
    assert got.dtype == F32
    rn.check(got, ref, f"fp32 {order} @ {name}")
    assert (np.diff(got, axis=1) >= 0).all()


def test_float64_value_lies_inside():
    for name in rn.CASE_NAMES:
        c, ref = _case(name)
        assert (rn.ratios(ref.value, ref) <= 1.0).all(), name


@pytest.mark.parametrize("name", [c[0] for c in rn.CASES if c[4] in rn.SHARP])
def test_ambiguity_cap(name):
    """A condition on the reference alone: on the sharp fields at most 5 % of
    the samples may have more than one allowed interval."""
    c, ref = _case(name)
    print(f"{name}: {ref.ambiguous:.2%} of {ref.n_allowed.size} samples with more than one interval")
    assert ref.ambiguous <= rn.AMBIGUITY_CAP


def test_degenerate_cases_are_present():
    fields = {c[4] for c in rn.CASES}
    assert fields == {"random", "sparse90", "x50", "spike", "zero", "threshold", "tightz", "zequal", "zmax"}
    assert {c[5] for c in rn.CASES} == {"random", "planted", "dup", "equal", "asc", "desc", "cdfhit", "low"}
    assert {c[6] for c in rn.CASES} == {1.0, 0.7, 3.0}
    assert {c[3] for c in rn.CASES} == {1, 3, 5, 9, 64}
    # the threshold field does what it is for: empty bins whose guard is ambiguous
    c, ref = _case("T700_t1000_thr")
    assert ref.ambiguous > 0.05


# the case of the GPU test that rejects each mistake
KILLED_BY = {
    "carry_lost_64": "T130_t129",
    "run_lost_64": "T129_t128",
    "drop_1e5": "T16_t3",
    "wsum_all": "T3_t1",
    "bins_are_z": "T4_t2",
    "no_denom_guard": "T700_t1000_thr",
    "above_unclamped": "T1024_t1024",
    "pad_leak": "T65_t40",
    "unsorted": "T63_t63",
    "scale_ignored": "T66_t65",
}


def test_every_mutant_is_accounted_for():
    assert set(KILLED_BY) | set(rn.EQUIVALENT) == set(rn.MUTANTS)
    assert not set(KILLED_BY) & set(rn.EQUIVALENT)


@pytest.mark.parametrize("mutant", list(KILLED_BY))
def test_mutant_is_caught(mutant):
    """The mistaken evaluation, in fp32 as a kernel would make it and in every
    summation order, leaves the intervals of the named case (or does not
    ascend): the GPU test would fail on such a kernel."""
    c, ref = _case(KILLED_BY[mutant])
    for order in rn.ORDERS:
        got = rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, order, (mutant,))
        assert rn.caught(got, ref), (mutant, order)
        assert not rn.caught(rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, order), ref)


def test_large_shapes_reject_lost_carries():
    """the shapes past 64 KiB of LDS see a lost carry too"""
    for name, mutants in (("T1024_t1025_sparse", ("carry_lost_64", "run_lost_64")),
                          ("T2048_t1024", ("run_lost_64",)),
                          ("T2048_t1024_tight", ("carry_lost_64", "run_lost_64"))):
        c, ref = _case(name)
        for m in mutants:
            assert rn.caught(rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, "chunk", (m,)), ref), (name, m)


@pytest.mark.parametrize("mutant", rn.EQUIVALENT)
def test_equivalent_mutant_cannot_show(mutant):
    """``drop_1e15`` and ``last_delta_prev`` change nothing this stage can
    show (resample_numpy.EQUIVALENT says why): on every case the mistaken fp32
    evaluation is the unmistaken one bit for bit, and even in float64, where
    1e-15 is not absorbed, it moves no sample by a hundredth of its bound.  No
    test of the output can catch them."""
    for name in rn.CASE_NAMES:
        c, ref = _case(name)
        good = rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, "seq")
        bad = rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, "seq", (mutant,))
        assert not rn.caught(bad, ref), name
        assert np.array_equal(good, bad), name
        # in float64, where 1e-15 is not absorbed, still far inside the bound
        bad64 = rn.resample(c.z, c.sigma, c.u, c.density_scale, mutant=(mutant,))
        e_min = np.nanmin(np.where(ref.OK, ref.E, np.nan), axis=0)
        assert (np.abs(bad64 - ref.value) <= 1e-2 * e_min).all(), name


def test_check_rejects_what_is_outside():
    c, ref = _case("T65_t40")
    good = rn.resample(c.z, c.sigma, c.u, c.density_scale, F32, "chunk").astype(np.float64)
    rn.check(good, ref, "self")
    for bad in (np.nan, np.inf):
        g = good.copy()
        g[1, 7] = bad
        with pytest.raises(rn.Mismatch):
            rn.check(g, ref, "non-finite")
    g = good.copy()
    g[2, 3] += 1e-3
    with pytest.raises(rn.Mismatch):
        rn.check(g, ref, "moved")
    with pytest.raises(rn.Mismatch):
        rn.check(good[:, :-1], ref, "shape")
