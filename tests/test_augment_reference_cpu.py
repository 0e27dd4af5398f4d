"""The augmentation reference (tests/augment_numpy.py) held against the oracle
and against itself, on the CPU:

* its float64 values are ``oracle.augment.data_aug`` run on float64 tensors
  (with the rotation matrix rounded to float32 first, which is the kernel's
  contract and what the oracle does on float32 tensors), labels equal outside
  the two-candidate set;
* ``oracle.augment.data_aug`` in float32 -- another order of the same
  operations: BLAS ``bmm``, no FMA, a float32 pairwise mean -- passes the SAME
  ``compare`` call the GPU tests make on every case with nothing exempt, worst
  err / bound per family recorded in ``WORST_CPU`` and printed;
* every deliberate mistake of ``augment_numpy.MUTANTS`` is rejected by that
  call on the cases named in ``KILLED_BY``;
* what stays invisible is stated and shown;
* the hue of the six primaries, the grey pixel and the wrap, by hand.
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import augment as oa
from tests import augment_numpy as an

F32, F64 = np.float32, np.float64
WORST_CPU = {}
SHARE = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if WORST_CPU:
        print("\nworst err / bound of the float32 oracle per case family:")
        for k in sorted(WORST_CPU):
            print(f"  {k}: {WORST_CPU[k]:.3f}")
    if SHARE:
        print("largest share of two-candidate label pixels per case family:")
        for k in sorted(SHARE):
            print(f"  {k}: {100 * SHARE[k]:.3f} %")


def _float32_matrix(angle_deg):
    return [float(F32(v)) for v in _double_matrix(angle_deg)]


_double_matrix = oa._inverse_rotation_matrix


def oracle(c, dtype):
    """``data_aug`` image by image on tensors of ``dtype`` -> image, label | None"""
    imgs, labs = [], []
    for b in range(c.B):
        p = c.params[b]
        lab = torch.zeros(c.H, c.W, dtype=torch.int64) if c.label is None else torch.from_numpy(c.label[b])
        i, l = oa.data_aug(torch.from_numpy(c.img[b]).to(dtype), lab, p["order"], an.f32(p["brightness"]),
                           an.f32(p["contrast"]), an.f32(p["saturation"]), an.f32(p["hue"]),
                           an.f32(p["angle_deg"]), p["flip"], (p["crop_i"], p["crop_j"]), c.out_size)
        imgs.append(i.numpy())
        labs.append(l.numpy())
    return np.stack(imgs), None if c.label is None else np.stack(labs)


@pytest.mark.parametrize("name", an.case_specs())
def test_float64_values_are_the_oracles(name, monkeypatch):
    monkeypatch.setattr(oa, "_inverse_rotation_matrix", _float32_matrix)
    c, ref = an.build_case(name), an.reference(name)
    img, lab = oracle(c, torch.float64)
    assert np.array_equal(np.isnan(img), np.isnan(ref.img))
    fin = np.isfinite(ref.img)
    assert np.array_equal(img[~fin], ref.img[~fin], equal_nan=True)
    assert float(np.abs(img[fin] - ref.img[fin]).max(initial=0.0)) <= 1e-12
    if lab is not None:
        single = (ref.cands == ref.cands[..., :1]).all(-1)
        assert np.array_equal(lab[single], ref.label[single])
        assert (lab[..., None] == ref.cands).any(-1).all()


@pytest.mark.parametrize("name", an.case_specs())
def test_float32_oracle_stays_inside_the_bounds(name):
    """if this fails the rounding count is wrong, not the oracle"""
    c, ref = an.build_case(name), an.reference(name)
    img, lab = oracle(c, torch.float32)
    fam = an.family_of(name)
    WORST_CPU[fam] = max(WORST_CPU.get(fam, 0.0), an.compare(img, lab, ref, f"float32 oracle {fam}", name))
    SHARE[fam] = max(SHARE.get(fam, 0.0), c.share)
    assert c.share <= an.MAX_LABEL_SHARE


def test_the_families_hold_what_they_are_for():
    orders = an.build_case("orders")
    assert sorted(tuple(p["order"]) for p in orders.params) == sorted(
        itertools.permutations(range(4)))
    assert all(p["contrast"] != 1 for p in orders.params) and orders.B == 24
    n_blk = lambda H, W: -(-H * W // 1024)
    assert [n_blk(H, W) for H, W in an.MEAN_SIZES] == [1, 1, 2, 2, 5]
    for name in an.case_specs("mean"):
        c = an.build_case(name)
        assert c.out_size[0] * c.out_size[1] != c.H * c.W or c.H * c.W == 1
    for name in an.case_specs("crop_flip"):
        c = an.build_case(name)
        assert (c.out_size[0] * c.out_size[1]) % 256 != 0
        assert {(p["crop_i"], p["crop_j"]) for p in c.params} == \
            {(0, 0), (c.H - c.out_size[0], c.W - c.out_size[1]), (3, 8)}
    # 45 degrees on 1 x 37: rows wholly out of frame come out as exact zeros, bound 0
    ref = an.reference("rotation_1x37_45")
    assert (ref.bound == 0).mean() > 0.5 and (ref.img[ref.bound == 0] == 0).all()
    # a quarter turn at unequal parity: every coordinate on a half-integer, image only
    c = an.build_case("rotation_16x23_90")
    ix, iy, _, _ = an.source_coords(c.H, c.W, c.H, c.W, c.params[0])
    assert c.label is None and np.allclose(ix % 1, 0.5, atol=1e-9) and np.allclose(iy % 1, 0.5, atol=1e-9)
    assert an.build_case("rotation_17x23_90").label is not None
    # the table's hand-placed pixels are what their names say
    tab, names = an.pixel_table()
    px = dict(zip(names, tab.reshape(3, -1).T))
    assert (px["grey"] == 0.5).all() and px["grey_g_ulp"][1] == np.nextafter(F32(0.5), F32(1))
    assert px["tie_rg"][0] == px["tie_rg"][1] > px["tie_rg"][2] and px["minc0"].min() == 0
    assert [tuple(px[f"primary{k}"]) for k in range(6)] == \
        [(1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 1)]


# ---------------------------------------------------------------------------
# sharpness: wrong implementations are rejected
# ---------------------------------------------------------------------------
# mutant -> the cases of the GPU module that reject it
KILLED_BY = {
    "grey_0299": ["orders", "mean_17x61_bc"],
    "mean_of_input": ["orders", "mean_3x343_hs"],
    "mean_tail_lost": ["mean_64x65_outlier", "mean_1x255_bc", "mean_3x343_outlier"],
    "mean_div_ohow": ["mean_17x61_bc", "mean_1x255_outlier"],
    "mean_wrong_b0": ["batch17", "batch33"],
    "params_first_launch": ["batch17", "orders"],
    "image_no_b0": ["batch33", "pixels"],
    "no_clamp": ["pixels", "mean_17x61_bc"],
    "hue_not_wrapped": ["pixels", "orders"],
    "sector_rounded": ["pixels"],
    "tie_green_first": ["pixels"],
    "no_eqc_guard": ["pixels"],
    "nan_clamped": ["nonfinite_nan_contrast_first", "nonfinite_nan_hue_first", "nonfinite_inf_contrast_first"],
    "flip_about_w": ["crop_flip", "crop_flip_ow1"],
    "flip_before_crop": ["crop_flip", "crop_flip_nolabel"],
    "crop_swapped": ["crop_flip", "mean_17x61_bc"],
    "rotation_sign": ["rotation_17x23_7.3", "rotation_16x23_-10"],
    "no_half": ["orders", "rotation_16x23_7.3"],
    "no_mask": ["rotation_17x23_7.3", "rotation_1x37_45"],
    "label_fill_0": ["rotation_1x37_45", "rotation_17x23_-10"],
    "label_floor": ["rotation_17x23_7.3", "rotation_24x40_-10"],
    "weights_swapped_x": ["rotation_17x23_7.3", "rotation_24x40_45"],
}


def _survives(mutant, case):
    """True when ``compare`` accepts the mutant's output on the case (a name or
    a Case)."""
    c = an.build_case(case) if isinstance(case, str) else case
    ref = an.reference(case) if isinstance(case, str) else an.evaluate(c)
    got = an.evaluate(c, None if mutant == "none" else mutant)
    try:
        an.compare(got.img, got.label, ref, "mutants", c.name)
    except an.Mismatch:
        return False
    return True


def test_mutant_table_is_complete():
    assert set(KILLED_BY) == set(an.MUTANTS)
    assert all(k in an.case_specs() for lst in KILLED_BY.values() for k in lst)


@pytest.mark.parametrize("mutant,case", [(m, k) for m, lst in KILLED_BY.items() for k in lst], ids=str)
def test_mutant_is_rejected(mutant, case):
    assert _survives("none", case), "the clean evaluation must pass the same call"
    assert not _survives(mutant, case), f"{mutant} passes {case}"


def test_what_the_cases_cannot_see():
    """* Labels by round-half-away instead of half-to-even: an exact half-integer
      coordinate occurs only where the reference is itself within delta of the
      tie, and there both neighbours are candidates.
    * A tie for the maximum resolved green-first CONSISTENTLY (red excluded where
      green claims it) is the same function: the hue is continuous across the
      change of the maximum channel.  ``tie_green_first`` of MUTANTS is the
      inconsistent form, where both claim it.
    * ``h + hue`` left unwrapped is the same function as long as the sector is
      reduced mod 6 from its floor; ``hue_not_wrapped`` of MUTANTS also loses the
      ``% 6``.
    * Which sector a NaN hue is given (torch: whatever int32(NaN) is on the host):
      p, q, t and v are NaN or inf, and the contrast op, which always runs,
      spreads a NaN over the image through the mean.
    * No crop hides a mean divided by oh * ow; P a multiple of 1024 hides the lost
      tail; B <= 16 hides everything about b0; no flip hides where the flip is.
    """
    some = ["pixels", "orders", "rotation_17x23_7.3", "rotation_16x23_90", "rotation_24x40_180",
            "crop_flip", "batch17"]
    for m in an.EQUIVALENT:
        for name in some:
            assert _survives(m, name), (m, name)
    assert _survives("mean_div_ohow", "orders")
    rng = np.random.default_rng(5)
    square = an.Case("32x32", an._noise(rng, 1, 32, 32), None, [an._param([0, 1, 2, 3], 1.3, 1.3, 0.7, 0.05)])
    assert _survives("mean_tail_lost", square)
    for m in ("mean_wrong_b0", "params_first_launch", "image_no_b0"):
        assert _survives(m, "batch16") and _survives(m, "batch1")
    for m in ("flip_about_w", "flip_before_crop"):
        assert _survives(m, "orders")
    assert _survives("no_mask", "orders") and _survives("rotation_sign", "rotation_24x40_180")
    # every coordinate on a half-integer: the weights are 1/2 and 1/2
    assert _survives("weights_swapped_x", "rotation_16x23_90")
    # one row, by = 0: iy = -+ sin * bx weighs row 0 by 1 - |iy| either way
    assert _survives("rotation_sign", "rotation_1x37_45")


# ---------------------------------------------------------------------------
# the hue op by hand
# ---------------------------------------------------------------------------
PRIMARIES = [(1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1), (1, 0, 1)]


def _shift(px, hue):
    return an.jitter(np.array([px], F64), an._param([3, 0, 1, 2], h=hue), mean=0.5)[0][0]


def test_hue_by_hand():
    # factors 1: brightness, contrast and saturation are the identity, hue first
    for k, px in enumerate(PRIMARIES):
        assert np.allclose(_shift(px, 0.0), px, atol=1e-12)
        # hue is k / 6: a shift by 1/6 is the next primary, by 1/2 the complement
        assert np.allclose(_shift(px, 1 / 6), PRIMARIES[(k + 1) % 6], atol=1e-7)
        assert np.allclose(_shift(px, -1 / 6), PRIMARIES[(k - 1) % 6], atol=1e-7)
        assert np.allclose(_shift(px, 0.5), PRIMARIES[(k + 3) % 6], atol=1e-7)
        assert np.allclose(_shift(px, -0.5), PRIMARIES[(k + 3) % 6], atol=1e-7)
    # a grey pixel has no hue to shift; neither has black or white
    for g in (0.0, 0.5, 1.0):
        for hue in (-0.5, -0.05, 0.05, 0.5):
            assert np.array_equal(_shift((g, g, g), hue), (g, g, g))
    # the wrap: hue 0.95 + 0.05 is red again, 0.05 - 0.05 too, and the values
    # just either side of the wrap are close to it
    for h, hue in ((0.95, 0.05), (0.05, -0.05), (0.5, 0.5), (0.5, -0.5)):
        for side in (-1e-9, 0.0, 1e-9):
            assert np.allclose(_shift(an.hsv_pixel(h + side, 1.0, 1.0), hue), (1, 0, 0), atol=1e-7)
    # half saturation, half value, a third of the way from red to yellow
    assert np.allclose(an.hsv_pixel(1 / 18, 0.5, 0.5), (0.5, 0.25 + 0.25 / 3, 0.25))
    assert np.allclose(_shift((0.5, 0.25 + 0.25 / 3, 0.25), 1 / 9), (0.5, 0.5, 0.25), atol=1e-12)


def test_nonfinite_values_propagate():
    px = np.array([[np.nan, 0.5, 0.25], [0.5, 0.25, 0.125]], F64)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 3, 0, 1]):
        out = an.jitter(px, an._param(order, 1.3, 1.3, 0.7, 0.05), mean=0.4)[0]
        assert np.isnan(out[0]).any() and np.isfinite(out[1]).all()
        assert np.isnan(an.jitter(px, an._param(order, 1.3, 1.3, 0.7, 0.05), mean=np.nan)[0]).all()
    ref = an.reference("nonfinite_nan_contrast_last")
    assert np.isnan(ref.img[0]).all() and np.isfinite(ref.img[1]).all()
    ref = an.reference("nonfinite_nan_rotated")          # out of frame stays an exact 0
    assert np.isnan(ref.img[0]).any() and (ref.img[0][~np.isnan(ref.img[0])] == 0).all()
    ref = an.reference("nonfinite_inf_contrast_first_white")
    assert np.isfinite(ref.img).all() and np.isfinite(ref.bound).all()
    ref = an.reference("nonfinite_inf_contrast_first")   # one NaN pixel's footprint in black
    assert 0 < np.isnan(ref.img[0]).sum() <= 3 * 9 and (ref.img[0][~np.isnan(ref.img[0])] == 0).all()
