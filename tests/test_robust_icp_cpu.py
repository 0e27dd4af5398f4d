"""CPU-only: the weighted ICP steps' restatement (tests/robust_numpy.py) held to
the plain restatements' words where the contract says they are equal, the
boundary rows of the weight, and what the robust kernels do to a frame that
shows something its target does not: the experiments behind the README's and
the notebook's figures (docs/DESIGN_NOTEBOOK.md, RB), rerun here on the
restatement.  tests/test_gpu_robust_icp.py holds the kernels to the same
restatement bit for bit."""
import inspect

import numpy as np
import pytest

from tests import projective_numpy as PJ
from tests import robust_numpy as RB
from tests import tsdf_register_numpy as TR
from tests.test_projective_cpu import (ROOM_ITERATIONS, ROOM_K, ROOM_PAIRS, path_case,
                                       render_room, room_gate, room_pair)
from tests.test_register_cpu import bits, pose_error
from tests.test_tsdf_register_cpu import ROOM_TRUNC, room_volume, twist
from ucsa_neural_rendering_amd.utils import registration as REG
from ucsa_neural_rendering_amd.utils.registration import compose

F = np.float32
_CACHE = {}


def words(a):
    return np.ascontiguousarray(a, F).view(np.int32)


# ---- the boundary rows of the weight: |r| is set exactly, on both routes -------------
P_VALUES = [0.0, -1.0, np.nan, np.inf, 1e-40, 1.0, 0.375, 2.5]     # 1e-40: a float32 denormal
SCALES = [0.125, 0.3]                                             # a power of two, and not


def boundary_abs(scale):
    """|r| at the scale, one ulp on each side of it, well inside and well outside"""
    s = F(scale)
    return np.array([s, np.nextafter(s, F(1)), np.nextafter(s, F(0)), F(0.5) * s, F(2.0) * s,
                     F(2.0) ** -20], F)


def boundary_rows(scale):
    """(a [N], p [N]): every |r| of ``boundary_abs`` with every point weight"""
    a = np.repeat(boundary_abs(scale), len(P_VALUES))
    p = np.tile(np.array(P_VALUES, F), len(boundary_abs(scale)))
    return a, p


def boundary_projective(scale):
    """a 1 x 1 target at the origin with normal -z and points (0, 0, a) under the
    identity: d = (0, 0, -a) and r = (0*0 + 0*0) + (-1)*(-a) = a, exactly"""
    a, p = boundary_rows(scale)
    pts = np.stack([np.zeros_like(a), np.zeros_like(a), a], 1)
    tp = np.zeros((1, 1, 3), F)
    tn = np.array([[[0.0, 0.0, -1.0]]], F)
    tm = np.array([[3]], np.uint8)
    return pts, tp, tn, tm, (1.0, 1.0, 0.5, 0.5), p, dict(max_dist=1.0)


def boundary_tsdf(scale):
    """a 2 x 2 x 2 lattice at the origin, spacing 1, tsdf 0 on the face i = 0 and 1 on
    i = 1, trunc 1, points (a, 0.5, 0.5): F = 0 + a*(1 - 0) = a, the gradient is
    (1, 0, 0) and r = -(a * 1) = -a, exactly"""
    a, p = boundary_rows(scale)
    tsdf = np.zeros((2, 2, 2), F)
    tsdf[1] = 1.0
    vol = {"tsdf": tsdf, "weight": np.ones((2, 2, 2), F), "rgb": None,
           "origin": np.zeros(3, F), "spacing": np.ones(3, F)}
    pts = np.stack([a, np.full_like(a, 0.5), np.full_like(a, 0.5)], 1)
    return vol, pts, p, dict(trunc=1.0)


def expected_weight(a, p, robust, scale):
    """the contract read off row by row, in Python floats rounded once per operation"""
    out = []
    s = F(scale)
    for ai, pi in zip(a, p):
        if robust == "none":
            rho = F(1.0)
        elif robust == "huber":
            rho = F(1.0) if ai <= s else s / ai
        else:
            t = ai / s
            u = F(1.0) - t * t
            rho = u * u if ai < s else F(0.0)
        ok = bool(pi > 0) and bool(np.isfinite(pi))
        out.append(F(pi * rho) if ok else F(0.0))
    return np.array(out, F)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("robust", ["none", "huber", "tukey"])
def test_the_boundary_rows_get_the_weight_the_contract_writes(robust, scale):
    a, p = boundary_rows(scale)
    with np.errstate(all="ignore"):
        want = expected_weight(a, p, robust, scale)
    # what the table must show, whatever the arithmetic: the scale itself, its two
    # neighbours, and the eight point weights
    at = lambda ai, pi: want[int(np.nonzero(boundary_abs(scale) == ai)[0][0]) * len(P_VALUES)
                             + P_VALUES.index(pi)]
    s = F(scale)
    up, down = np.nextafter(s, F(1)), np.nextafter(s, F(0))
    if robust == "huber":
        assert at(s, 1.0) == 1.0 and at(down, 1.0) == 1.0 and 0.0 < at(up, 1.0) < 1.0
        assert at(F(2.0) * s, 2.5) == F(1.25)
    if robust == "tukey":
        assert at(s, 1.0) == 0.0 and at(up, 1.0) == 0.0 and at(down, 1.0) > 0.0
        assert at(F(0.5) * s, 1.0) == F(0.5625)
    if robust != "tukey":
        assert at(F(2.0) ** -20, 1e-40) == F(1e-40) > 0        # a denormal weight still counts
    for ai in boundary_abs(scale):
        for bad in (0.0, -1.0, np.inf):
            assert words(at(ai, bad)) == 0
    nan_rows = np.isnan(p)
    assert (words(want[nan_rows]) == 0).all()
    # both routes produce exactly these weights from exactly these residuals
    pts, tp, tn, tm, K, pw, kw = boundary_projective(scale)
    sums, pixel, residual, w = RB.projective_sums_weighted(
        pts, None, tp, tn, tm, K, np.eye(4), kw["max_dist"], point_weight=pw, robust=robust,
        robust_scale=scale)
    assert (pixel == 0).all() and np.array_equal(words(residual), words(a))
    assert np.array_equal(words(w), words(want))
    assert sums[28] == (want > 0).sum()
    vol, vpts, pw, kw = boundary_tsdf(scale)
    vsums, value, matched, vw = RB.tsdf_sums_weighted(vol, vpts, np.eye(4), kw["trunc"],
                                                      point_weight=pw, robust=robust,
                                                      robust_scale=scale)
    assert matched.all() and np.array_equal(words(value), words(a))
    assert np.array_equal(words(vw), words(want))
    assert vsums[28] == (want > 0).sum()
    # slot 27 is sum w r^2: against float64 from the weights, to the rounding of sqrt(w)^2
    ref = float((want.astype(np.float64) * a.astype(np.float64) ** 2).sum())
    assert abs(sums[27] - ref) <= 4 * 2.0 ** -24 * ref and abs(vsums[27] - ref) <= 4 * 2.0 ** -24 * ref


def test_rows_that_do_not_count_are_positive_zero_everywhere():
    a, p = boundary_rows(0.125)
    r = (-a).astype(F)
    J = [np.full_like(a, v) for v in (-0.5, 0.25, -2.0, 0.6, -0.0, -0.8)]
    matched = np.ones(a.size, bool)
    matched[::5] = False
    for robust in ("none", "huber", "tukey"):
        counts, Js, rs, w = RB.weighted_rows(matched, J, r, p, robust, 0.125)
        off = ~counts
        assert off.sum() > 10 and counts.sum() > 5
        for x in Js + [rs, w]:
            assert x.dtype == F and (words(x[off]) == 0).all()
        terms = TR.point_terms(counts, Js, rs)
        assert (terms[off].view(np.int64) == 0).all()
        # a row counts iff it matched and its weight is positive
        with np.errstate(all="ignore"):
            assert np.array_equal(counts, matched & (RB.robust_weight(r, p, robust, 0.125) > 0))
    # NaN residuals of unmatched rows do not leak
    r[0], J[0][0] = np.nan, np.inf
    matched[0] = False
    counts, Js, rs, w = RB.weighted_rows(matched, J, r, None, "huber", 0.125)
    assert not counts[0] and words(w[:1])[0] == 0 and np.isfinite(TR.point_terms(counts, Js, rs)).all()


# ---- equality with the plain restatements, as words -------------------------------------
def test_without_weights_the_projective_sums_are_the_plain_restatements_words():
    from tests.test_gpu_projective import TRANSFORMS, source_points, target_maps
    tp, tn, tm, K = target_maps("17x33")
    for tname, T in TRANSFORMS.items():
        src, nrm = source_points(tp, 257, T, 7)
        # reject 4: nearly every pixel of this wavy surface carries the GRAZING bit
        plain = PJ.projective_sums(src, nrm, tp, tn, tm, K, T, 0.3, 0.5, 4)
        assert plain[0][28] > 50
        with np.errstate(all="ignore"):
            biggest = float(np.nanmax(np.abs(plain[2]))) if np.isfinite(plain[2]).any() else 1.0
        cases = [dict(), dict(point_weight=np.ones(257, F)),
                 dict(robust="huber", robust_scale=biggest),
                 dict(robust="huber", robust_scale=2.0 * biggest, point_weight=np.ones(257, F))]
        for kw in cases:
            got = RB.projective_sums_weighted(src, nrm, tp, tn, tm, K, T, 0.3, 0.5, 4, **kw)
            assert bits(got[0]).tolist() == bits(plain[0]).tolist(), (tname, kw)
            assert np.array_equal(got[1], plain[1])
            assert np.array_equal(words(got[2]), words(plain[2]))
            assert np.array_equal(got[3] == 1.0, plain[1] >= 0) and set(got[3]) <= {F(0), F(1)}


def test_without_weights_the_tsdf_sums_are_the_plain_restatements_words():
    from tests.test_gpu_tsdf_register import TRANSFORMS, random_volume, source_of, world_points
    vol = random_volume("small")
    world = world_points(vol, 257, 457)
    for tname, T in TRANSFORMS.items():
        src = source_of(world, T)
        plain = TR.tsdf_sums(vol, src, T, 0.3, 1.0, 0.5)
        assert plain[0][28] > 10
        cases = [dict(), dict(point_weight=np.ones(257, F)),
                 dict(robust="huber", robust_scale=0.5 * 0.3),          # |r| <= max_tsdf * trunc
                 dict(robust="huber", robust_scale=1.0, point_weight=np.ones(257, F))]
        for kw in cases:
            got = RB.tsdf_sums_weighted(vol, src, T, 0.3, 1.0, 0.5, **kw)
            assert bits(got[0]).tolist() == bits(plain[0]).tolist(), (tname, kw)
            assert np.array_equal(words(got[1]), words(plain[1]))
            assert np.array_equal(got[2], plain[2])
            assert np.array_equal(got[3] == 1.0, plain[2] == 1)


def test_with_the_defaults_the_restated_loops_end_where_the_plain_loops_end():
    _, _, src, dst, true = room_pair("pillar")
    init = compose(true, twist(2.0, 0.03, 0))
    a = PJ.register_frames(src, dst, ROOM_K, init=init, iterations=(3, 2, 2))
    b = RB.register_frames(src, dst, ROOM_K, init=init, iterations=(3, 2, 2))
    assert bits(a["transform"]).tolist() == bits(b["transform"]).tolist()
    assert all(bits(x["sums"]).tolist() == bits(y["sums"]).tolist()
               for x, y in zip(a["history"], b["history"]))
    pts = TR.backproject(render_room(room_pair("pillar")[0]), ROOM_K)[::7]
    start = compose(room_pair("pillar")[0], twist(2.0, 0.03, 0))
    a = TR.register_points_tsdf(pts, room_volume(), ROOM_TRUNC, init=start, iterations=3)
    b = RB.register_points_tsdf(pts, room_volume(), ROOM_TRUNC, init=start, iterations=3)
    assert bits(a["transform"]).tolist() == bits(b["transform"]).tolist()


# ---- a frame that shows something its target does not ---------------------------------
# rows, columns and how much nearer the block's pixels are: inside max_dist 0.3 (and,
# at 0.15, inside the truncation band 0.2 of the TSDF route)
BLOCKS = {"16%": ((20, 45, 25, 55), 0.15), "6%": ((25, 40, 30, 50), 0.2)}
TUKEY_C, TUKEY_C_TSDF, HUBER_K = 0.08, 0.05, 0.02
START = (2.0, 0.03, 0)                                   # degrees, units, the twist's seed
TSDF_ITERATIONS = 15

# Measured with this restatement, 60 x 80 frames, iterations (10, 5, 4), max_dist 0.3,
# min_cos 0.8, start 2 deg / 0.03 (seed 0): (rotation, translation) error of the end in
# (radians, units).  "clean" is the frame without a block.
MEASURED = {
    ("pillar", "16%"): {"plain": (2.423e-2, 2.973e-2), "tukey": (1.555e-4, 3.361e-4),
                        "huber": (5.789e-3, 7.284e-3)},
    ("pillar", "6%"): {"plain": (1.588e-2, 1.995e-2), "tukey": (1.625e-4, 3.639e-4),
                       "huber": (2.844e-3, 3.666e-3)},
    ("corner", "16%"): {"plain": (5.488e-2, 1.091e-1), "tukey": (2.096e-4, 1.847e-3),
                        "huber": (2.213e-2, 5.088e-2)},
    ("corner", "6%"): {"plain": (5.103e-2, 1.719e-1), "tukey": (1.803e-4, 1.817e-3),
                       "huber": (1.069e-2, 2.284e-2)},
    ("pillar", "clean"): {"tukey": (1.864e-4, 3.885e-4), "huber": (1.890e-4, 3.978e-4)},
    ("corner", "clean"): {"tukey": (1.342e-4, 1.768e-3), "huber": (1.359e-4, 1.789e-3)},
}
# the TSDF route: room_volume() (voxel 0.05, trunc 0.2), the pillar pair's source view
# (4 800 points), 15 iterations, the same start; the clean plain end is (3.401e-4, 7.088e-4)
MEASURED_TSDF = {
    "16%": {"plain": (2.145e-2, 4.772e-2), "tukey": (2.734e-4, 6.108e-4),
            "huber": (5.654e-3, 1.256e-2)},
    "6%": {"plain": (1.742e-2, 3.404e-2), "tukey": (2.627e-4, 5.909e-4),
           "huber": (2.854e-3, 5.853e-3)},
    "clean": {"plain": (3.401e-4, 7.088e-4), "tukey": (3.315e-4, 6.941e-4),
              "huber": (3.401e-4, 7.089e-4)},
}


def blocked(depth, block):
    (r0, r1, c0, c1), off = BLOCKS[block]
    out = depth.copy()
    out[r0:r1, c0:c1] -= F(off)
    return out


def blocked_maps(name, block):
    key = ("maps", name, block)
    if key not in _CACHE:
        _CACHE[key] = PJ.frame_maps(blocked(render_room(room_pair(name)[0]), block), ROOM_K,
                                    levels=3)
    return _CACHE[key]


def run_frames(name, block, init=None, **kw):
    _, _, src, dst, true = room_pair(name)
    if block != "clean":
        src = blocked_maps(name, block)
    init = compose(true, twist(*START)) if init is None else init
    out = RB.register_frames(src, dst, ROOM_K, init=init, iterations=ROOM_ITERATIONS,
                             max_dist=0.3, min_cos=0.8, **kw)
    return pose_error(out["transform"], true), out


@pytest.mark.parametrize("block", sorted(BLOCKS))
@pytest.mark.parametrize("name", sorted(ROOM_PAIRS))
def test_a_moved_block_biases_the_plain_loop_and_tukey_ends_inside_the_clean_gate(name, block):
    gate_rot, gate_trans = room_gate(name)
    (prot, ptrans), plain = run_frames(name, block)
    (trot, ttrans), tukey = run_frames(name, block, robust="tukey", robust_scale=TUKEY_C)
    (hrot, htrans), huber = run_frames(name, block, robust="huber", robust_scale=HUBER_K)
    print(f"{name} {block}: plain {prot:.3e} / {ptrans:.3e}, tukey {trot:.3e} / {ttrans:.3e} "
          f"(counted {tukey['matched']} of {tukey['n_points']}), huber {hrot:.3e} / {htrans:.3e}; "
          f"gate {gate_rot:.3e} / {gate_trans:.3e}; recorded {MEASURED[name, block]}")
    assert plain["rank"] == tukey["rank"] == 6
    assert prot > 10.0 * gate_rot                      # otherwise the fixture shows nothing
    assert trot <= gate_rot and ttrans <= gate_trans
    assert tukey["history"][-1]["robust"] == "tukey"
    assert tukey["history"][-1]["robust_scale"] == TUKEY_C
    # Huber bounds the pull and does not remove it: on record, no gate
    assert np.isfinite(hrot) and huber["rank"] == 6


@pytest.mark.parametrize("robust,scale", [("tukey", TUKEY_C), ("huber", HUBER_K)])
@pytest.mark.parametrize("name", sorted(ROOM_PAIRS))
def test_on_clean_frames_both_kernels_end_inside_the_clean_gate(name, robust, scale):
    gate_rot, gate_trans = room_gate(name)
    (rot, trans), out = run_frames(name, "clean", robust=robust, robust_scale=scale)
    print(f"{name} clean, {robust} {scale}: {rot:.3e} / {trans:.3e}, counted {out['matched']} "
          f"of {out['n_points']}; recorded {MEASURED[name, 'clean'][robust]}")
    assert out["rank"] == 6 and rot <= gate_rot and trans <= gate_trans


def run_tsdf(block, **kw):
    src_pose = room_pair("pillar")[0]
    depth = render_room(src_pose)
    pts = TR.backproject(depth if block == "clean" else blocked(depth, block), ROOM_K)
    out = RB.register_points_tsdf(pts, room_volume(), ROOM_TRUNC, iterations=TSDF_ITERATIONS,
                                  init=compose(src_pose, twist(*START)), **kw)
    return pose_error(out["transform"], src_pose), out


def tsdf_clean_gate():
    """twice the clean frame's plain end from the same start"""
    if "tsdf gate" not in _CACHE:
        (rot, trans), _ = run_tsdf("clean")
        _CACHE["tsdf gate"] = (2.0 * rot, 2.0 * trans)
    return _CACHE["tsdf gate"]


@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_the_tsdf_route_with_a_moved_block(block):
    gate_rot, gate_trans = tsdf_clean_gate()
    (prot, ptrans), plain = run_tsdf(block)
    (trot, ttrans), tukey = run_tsdf(block, robust="tukey", robust_scale=TUKEY_C_TSDF)
    (hrot, htrans), huber = run_tsdf(block, robust="huber", robust_scale=HUBER_K)
    print(f"TSDF route {block}: plain {prot:.3e} / {ptrans:.3e}, tukey {trot:.3e} / {ttrans:.3e} "
          f"(counted {tukey['matched']} of {tukey['n_points']}), huber {hrot:.3e} / {htrans:.3e}; "
          f"gate {gate_rot:.3e} / {gate_trans:.3e}; recorded {MEASURED_TSDF[block]}")
    assert plain["rank"] == tukey["rank"] == 6
    assert prot > 10.0 * gate_rot
    assert trot <= gate_rot and ttrans <= gate_trans
    assert np.isfinite(hrot) and huber["rank"] == 6


@pytest.mark.parametrize("robust,scale", [("tukey", TUKEY_C_TSDF), ("huber", HUBER_K)])
def test_the_tsdf_route_on_the_clean_frame_ends_inside_the_clean_gate(robust, scale):
    gate_rot, gate_trans = tsdf_clean_gate()
    (rot, trans), out = run_tsdf("clean", robust=robust, robust_scale=scale)
    print(f"TSDF route clean, {robust} {scale}: {rot:.3e} / {trans:.3e}; recorded "
          f"{MEASURED_TSDF['clean'][robust]}")
    assert out["rank"] == 6 and rot <= gate_rot and trans <= gate_trans


# ---- on record, without a gate: the basin -------------------------------------------------
PER_LEVEL_C = (0.08, 0.16, 0.32)


def test_the_wide_starts_and_the_per_level_schedule_are_on_record():
    """Tukey narrows the basin.  From 8 deg / 0.2 (seeds 0..2 of the twist) on the
    clean pairs, the ends in units of translation, as this test prints them:

        pair    seed  plain     tukey c=0.08  tukey c=(0.08, 0.16, 0.32)
        pillar  0     3.98e-4   1.78e-1       3.88e-4
        pillar  1     3.98e-4   3.88e-4       3.88e-4
        pillar  2     3.98e-4   3.28e-1       3.88e-4
        corner  0     1.79e-3   1.25e-1       1.77e-3
        corner  1     1.79e-3   2.07e-1       1.77e-3
        corner  2     3.69e-1   8.12e-1       3.69e-1

    A fixed c = 0.08 loses four of the five starts the plain loop brings home;
    corner 2 is lost to the plain loop as well.  The schedule, c doubled per
    level, brings all four back.  But from the tracking start 2 deg / 0.03 with
    the 16 % block the same schedule ends 2.71e-1 units away on the corner pair
    where the fixed c ends 1.85e-3: at c = 0.32 the block's 0.15 is an inlier on
    the coarsest level and the loop slides to a wrong minimum (with the 6 %
    block, and on the pillar pair with either, both end at the same place).  So
    the kernels are for the tracking regime, and a schedule is the caller's
    risk.  No gate: the figures are a record."""
    for name in sorted(ROOM_PAIRS):
        true = room_pair(name)[4]
        for seed in range(3):
            init = compose(true, twist(8.0, 0.2, seed))
            ends = [run_frames(name, "clean", init=init, **kw)[0][1] for kw in (
                {}, dict(robust="tukey", robust_scale=TUKEY_C),
                dict(robust="tukey", robust_scale=PER_LEVEL_C))]
            print(f"8 deg / 0.2, {name} seed {seed}: plain {ends[0]:.3e}, tukey c=0.08 "
                  f"{ends[1]:.3e}, per level {ends[2]:.3e}")
            assert np.isfinite(ends).all()
        for block in sorted(BLOCKS):
            fixed = run_frames(name, block, robust="tukey", robust_scale=TUKEY_C)[0]
            level = run_frames(name, block, robust="tukey", robust_scale=PER_LEVEL_C)[0]
            print(f"2 deg / 0.03, {name} {block}: tukey c=0.08 {fixed[0]:.3e} / {fixed[1]:.3e}, "
                  f"per level {level[0]:.3e} / {level[1]:.3e}")
            assert np.isfinite(fixed + level).all()


# ---- noisy odometry: do the weights help? -----------------------------------------------
def test_noisy_odometry_with_view_weights_and_huber_is_not_worse_than_the_seeds_spread():
    """The path of tests/test_projective_cpu.py through simulate_sensor_noise(sigma0
    0.002, sigma_z2 0.002, flying_share 0.5, jump 0.1), three levels (10, 5, 4), the
    last of 8 frames against the truth.  As this test prints them (rad / units):

        noise seed      0         1         2         3         4
        plain, units    3.83e-2   1.87e-2   2.44e-2   3.31e-2   4.98e-2
        view weights    3.44e-2   1.42e-2   1.67e-2   1.60e-2   5.21e-2

        seed 3: plain                                         3.140e-2 / 3.313e-2
                view weights (the noise model's own sigmas)   1.467e-2 / 1.603e-2
                huber, k = 1.345 * 0.01                       2.577e-2 / 2.985e-2
                both                                          1.492e-2 / 1.822e-2

    On seed 3 every variant ends nearer than the plain loop, the view weights at
    half its drift.  That is not yet evidence: the plain loop's own drift spreads
    over 3.1e-2 units across the five noise seeds, more than any of these
    differences, and over the five seeds the view weights win four times and lose
    once (mean 2.67e-2 against 3.29e-2).  The record says: they do not hurt, and
    whether they help is inside the noise of this sequence.  The gate is only
    that: not worse than plain by more than the spread over the seeds."""
    from ucsa_neural_rendering_amd.utils.depth_frontend import ViewWeights, simulate_sensor_noise
    depths, truth = path_case()
    noise = lambda seed: list(simulate_sensor_noise(depths, seed=seed, sigma0=0.002,
                                                    sigma_z2=0.002, flying_share=0.5, jump=0.1))
    vw = ViewWeights(sigma_depth=0.002, sigma_z2=0.002)
    plain, weighted = {}, {}
    for seed in range(5):
        poses, _, fallbacks = PJ.odometry(noise(seed), ROOM_K, iterations=ROOM_ITERATIONS)
        plain[seed] = pose_error(poses[-1], truth[-1])
        assert fallbacks == 0
        poses, _, fallbacks = RB.odometry(noise(seed), ROOM_K, iterations=ROOM_ITERATIONS,
                                          view_weights=vw)
        weighted[seed] = pose_error(poses[-1], truth[-1])
        assert fallbacks == 0
    spread_rot = max(r for r, _ in plain.values()) - min(r for r, _ in plain.values())
    spread_trans = max(t for _, t in plain.values()) - min(t for _, t in plain.values())
    show = lambda d: ", ".join(f"{r:.3e} / {t:.3e}" for r, t in d.values())
    print(f"plain, noise seeds 0..4: {show(plain)}; spread {spread_rot:.3e} / {spread_trans:.3e}")
    print(f"view weights, seeds 0..4: {show(weighted)}; mean translation "
          f"{np.mean([t for _, t in weighted.values()]):.3e} against "
          f"{np.mean([t for _, t in plain.values()]):.3e}")
    k = REG.robust_scale_for("huber", 0.01)           # sigma at z = 2: 0.002 + 0.002 * 4
    ends = {"view weights": weighted[3]}
    for label, kw in (("huber", dict(robust="huber", robust_scale=k)),
                      ("both", dict(view_weights=vw, robust="huber", robust_scale=k))):
        poses, _, fallbacks = RB.odometry(noise(3), ROOM_K, iterations=ROOM_ITERATIONS, **kw)
        ends[label] = pose_error(poses[-1], truth[-1])
        assert fallbacks == 0
    for label, (rot, trans) in ends.items():
        print(f"seed 3, {label}: {rot:.3e} / {trans:.3e} (plain {plain[3][0]:.3e} / "
              f"{plain[3][1]:.3e})")
        assert rot <= plain[3][0] + spread_rot and trans <= plain[3][1] + spread_trans


# ---- the host half ------------------------------------------------------------------------
def test_the_scale_helpers():
    assert REG.robust_scale_for("huber", 0.01) == 1.345 * 0.01
    assert REG.robust_scale_for("tukey", 2.0) == 4.685 * 2.0
    for bad in (("none", 1.0), ("cauchy", 1.0), ("huber", 0.0), ("tukey", float("nan"))):
        with pytest.raises(ValueError):
            REG.robust_scale_for(*bad)
    assert REG.robust_schedule("none", None) == [None]
    assert REG.robust_schedule("none", 0.3, 3) == [None] * 3
    assert REG.robust_schedule("tukey", 0.08, 3) == [0.08] * 3
    assert REG.robust_schedule("tukey", (0.08, 0.16, 0.32), 3) == [0.08, 0.16, 0.32]
    assert REG.robust_schedule("huber", [0.1, 0.05]) == [0.1, 0.05]
    for bad in (("tukey", None, 3), ("tukey", (0.1, 0.2), 3), ("huber", -1.0, None),
                ("huber", float("inf"), None), ("welsch", 1.0, None)):
        with pytest.raises(ValueError):
            REG.robust_schedule(*bad)


def test_the_keywords_are_opt_in_and_the_flat_surface_is_unchanged():
    from ucsa_neural_rendering_amd import ops
    assert not hasattr(ops, "projective_sums_weighted") and not hasattr(ops, "tsdf_sums_weighted")
    sig = inspect.signature(ops.register.projective_sums_weighted).parameters
    assert list(sig) == ["points", "normals", "target_points", "target_normals", "target_mask",
                         "intrinsics", "transform", "max_dist", "min_cos", "reject",
                         "point_weight", "robust", "robust_scale", "return_matches"]
    sig = inspect.signature(ops.register.tsdf_sums_weighted).parameters
    assert list(sig) == ["volume", "points", "transform", "trunc", "min_weight", "max_tsdf",
                         "point_weight", "robust", "robust_scale", "return_matches"]
    for fn in (ops.register.projective_sums_weighted, ops.register.tsdf_sums_weighted,
               REG.register_frames, REG.register_points_tsdf):
        p = inspect.signature(fn).parameters
        assert p["robust"].default == "none" and p["robust_scale"].default is None
        assert p["point_weight"].default is None
    assert inspect.signature(REG.register_frames).parameters["view_weights"].default is None
    assert ops.register.ROBUST == {"none": 0, "huber": 1, "tukey": 2}


# ---- the library's argument checks: before any launch, so they run without a GPU ----------
def test_every_argument_index_is_returned_before_any_launch():
    import ctypes as C

    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    host = (C.c_float * 64)()                  # never dereferenced: every call below is refused
    ptr = C.c_void_p(C.addressof(host))
    T12 = (C.c_float * 12)(*np.eye(4)[:3].reshape(-1))
    nan, inf = float("nan"), float("inf")
    good = dict(points=ptr, normals=ptr, n=257, tp=ptr, tn=ptr, tm=ptr, H=3, W=4, reject=12,
                fx=2.0, fy=2.0, cx=0.5, cy=0.25, T=T12, md=0.3, mc=0.5, pw=ptr, kind=2, scale=0.1,
                ws=ptr, wsn=58, sums=ptr)

    def proj(**over):
        a = {**good, **over}
        return l.ucsa_projective_icp_sums_weighted(
            a["points"], a["normals"], a["n"], a["tp"], a["tn"], a["tm"], a["H"], a["W"],
            a["reject"], a["fx"], a["fy"], a["cx"], a["cy"], a["T"], a["md"], a["mc"], a["pw"],
            a["kind"], a["scale"], a["ws"], a["wsn"], a["sums"], None, None, None, None)
    cases = [(0, dict(points=None)), (2, dict(n=0x80000000)), (3, dict(tp=None)),
             (4, dict(tn=None)), (5, dict(tm=None)), (6, dict(H=0)), (6, dict(H=16385)),
             (7, dict(W=0)), (7, dict(W=16385)), (8, dict(reject=1)), (8, dict(reject=16)),
             (9, dict(fx=0.0)), (9, dict(fx=nan)), (10, dict(fy=inf)), (11, dict(cx=nan)),
             (12, dict(cy=-inf)), (13, dict(T=None)), (14, dict(md=0.0)), (14, dict(md=2e19)),
             (15, dict(mc=-1.5)), (15, dict(mc=nan)),
             (17, dict(kind=3)), (17, dict(kind=-1)), (18, dict(scale=0.0)),
             (18, dict(scale=-0.1)), (18, dict(scale=nan)), (18, dict(scale=inf)),
             (18, dict(kind=1, scale=nan)),
             (19, dict(ws=None)), (20, dict(wsn=57)), (21, dict(sums=None))]
    for k, over in cases:
        assert proj(**over) == -1000 - k, (k, over)
    # with kind 0 the scale is not read: the next check answers
    assert proj(kind=0, scale=nan, sums=None) == -1021
    o3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    h3 = (C.c_float * 3)(0.1, 0.1, 0.1)
    good = dict(tsdf=ptr, weight=ptr, nx=4, ny=5, nz=6, o=o3, h=h3, points=ptr, n=257, T=T12,
                trunc=0.3, mw=1.0, mt=1.0, pw=ptr, kind=1, scale=0.1, ws=ptr, wsn=58, sums=ptr)

    def tsdf(**over):
        a = {**good, **over}
        return l.ucsa_tsdf_icp_sums_weighted(
            a["tsdf"], a["weight"], a["nx"], a["ny"], a["nz"], a["o"], a["h"], a["points"], a["n"],
            a["T"], a["trunc"], a["mw"], a["mt"], a["pw"], a["kind"], a["scale"], a["ws"],
            a["wsn"], a["sums"], None, None, None, None)
    bad_h = (C.c_float * 3)(0.1, 0.0, 0.1)
    bad_o = (C.c_float * 3)(0.0, nan, 0.0)
    cases = [(0, dict(tsdf=None)), (1, dict(weight=None)), (2, dict(nx=1)),
             (2, dict(nx=2048, ny=2048, nz=512)), (3, dict(ny=1)), (4, dict(nz=1)),
             (5, dict(o=None)), (5, dict(o=bad_o)), (6, dict(h=None)), (6, dict(h=bad_h)),
             (7, dict(points=None)), (8, dict(n=0x80000000)), (9, dict(T=None)),
             (10, dict(trunc=0.0)), (10, dict(trunc=inf)), (11, dict(mw=0.0)), (11, dict(mw=nan)),
             (12, dict(mt=0.0)), (12, dict(mt=1.5)), (12, dict(mt=nan)),
             (14, dict(kind=3)), (14, dict(kind=-2)), (15, dict(scale=0.0)),
             (15, dict(scale=nan)), (15, dict(kind=2, scale=inf)),
             (16, dict(ws=None)), (17, dict(wsn=57)), (18, dict(sums=None))]
    for k, over in cases:
        assert tsdf(**over) == -1000 - k, (k, over)
    assert tsdf(kind=0, scale=-1.0, sums=None) == -1018
    for name in ("ucsa_projective_icp_sums_weighted", "ucsa_tsdf_icp_sums_weighted"):
        assert sorted(_lib.SIGNATURES).count(name) == 1
