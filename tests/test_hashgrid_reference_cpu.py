"""tests/hashgrid_numpy.py (the float64 yardstick of the hash-grid encode and of
its table gradient) held against the oracle and against itself, on the CPU:

* ``encode`` against ``oracle.field.hashgrid_encode`` and ``grad`` against its
  autograd, within the fp32 budgets the GPU tests use -- and plain fp32
  sequential accumulation of the same formula stays inside them too, so the
  budgets are not tighter than what fp32 arithmetic can do;
* sharpness: deliberately wrong references (a wrap at res^3, a dropped corner,
  swapped hash primes, cells from a float64 position, shifted fine-pass rows)
  are each rejected by the comparison the GPU tests call -- that comparison
  would notice those kernel bugs;
* the far faces of the box, stated as facts with hand-computed indices.
"""
import numpy as np
import pytest
import torch

from oracle import field as ofield
from tests import hashgrid_numpy as hn

GRIDS = {
    # the production table: per_level_scale = exp2(log2(2048 * bound / 16) / 15)
    "P": (4.0, dict()),
    # small: 4096-entry levels (two corners of a cell collide all the time)
    "S": (4.0, dict(n_levels=8, log2_hashmap_size=12, per_level_scale=2.0)),
    # 2 * bound not a power of two: the division branch of the unit mapping
    "D": (3.0, dict(n_levels=8, log2_hashmap_size=12, per_level_scale=2.0)),
}
SETS = ("faces", "box", "one_cell")
_cache = {}


def grid(name):
    if ("grid", name) not in _cache:
        bound, kw = GRIDS[name]
        spec = ofield.make_grid_spec(bound, **kw)
        _cache["grid", name] = (spec, hn.levels_of(spec), bound)
    return _cache["grid", name]


def points(gname, sname):
    _, levels, bound = grid(gname)
    if sname == "faces":
        return hn.points_faces(bound)
    if sname == "box":
        return hn.points_box(5000 if gname == "P" else 2049, bound, 11)
    return hn.points_one_cell(levels, bound)


def case(gname, sname):
    """(points, corners, d_feat, reference gradient), computed once."""
    key = ("case", gname, sname)
    if key not in _cache:
        _, levels, bound = grid(gname)
        x = points(gname, sname)
        corners = hn.level_corners(levels, bound, x)
        d_feat = hn.d_feat_for(len(levels), x.shape[0], 21)
        _cache[key] = (x, corners, d_feat, hn.grad_from(corners, d_feat))
    return _cache[key]


def test_level_tables_are_the_ones_the_cases_need():
    _, P, _ = grid("P")
    assert P[4][4] and P[4][0] < hn.BIN_SCALE          # hashed, below the bin threshold
    assert list(hn.binned_levels(P)) == [False] * 5 + [True] * 11
    assert P[1][1:4] == (25, 15632, 4096) and not P[1][4]
    assert P[2][1:3] == (37, 50656) and 37 ** 3 == 50653     # entries != res^3
    _, S, _ = grid("S")
    assert [lv[4] for lv in S] == [False] + [True] * 7 and all(lv[2] == 4096 for lv in S)
    assert list(hn.binned_levels(S)) == [False] * 3 + [True] * 5
    assert hn.p64_value_bits(1 << 19) == 26 and hn.p64_value_bits(4096) == 30


def test_point_sets_have_the_edges_they_claim():
    _, P, b = grid("P")
    f = hn.points_faces(b)
    assert f.shape == (609, 3) and float(np.abs(f).max()) == b
    on_face = (np.abs(f) == b).sum(1)
    assert all(int((on_face == k).sum()) >= 8 for k in (1, 2, 3))
    assert int((f == 0).all(1).sum()) == 1 and int(((f == 0).sum(1) == 1).sum()) >= 30
    # frac = 0 exactly at a zero coordinate on the odd-integer-scale levels
    _, frac = hn.cell_frac(hn.unit_coords(np.zeros((1, 3), np.float32), b), P[0][0])
    assert (frac == 0).all()
    oc = hn.points_one_cell(P, b)
    cell, _ = hn.cell_frac(hn.unit_coords(oc, b), P[-1][0])
    assert oc.shape[0] == 4099 and len(np.unique(cell, axis=0)) == 1
    o, d, z = hn.rays_case(b)
    p = hn.ray_points(o, d, z, hn.aabb_of(b))
    assert p.shape == (37 * 70, 3) and float(np.abs(p).max()) == b
    assert int((p == b).any(1).sum()) > 50 and int((p == -b).any(1).sum()) > 50
    assert (p[:350] == p[0]).all()                      # one run over five rays
    o, d, z_c, z_f, src = hn.merged_case(b)
    both = np.concatenate([z_c, z_f], 1)
    assert (np.diff(np.take_along_axis(both, src.astype(np.int64), 1), axis=1) >= 0).all()


def test_far_face_entries_are_what_the_formula_says():
    """A coordinate at +bound: x01 = 1, pos = scale + 0.5.  On level 1 of the
    production table (scale 23.25, res 25, 15632 entries) the +1 corner is
    24 = res - 1, the last cell of the row: (24, 24, 24) -> 24 + 24 * 25 +
    24 * 625 = 15624.  On level 2 (scale 35.76, res 37, 37^3 = 50653 rounded up
    to 50656 entries) pos = 36.26 and the +1 corner is 37 = res, outside the
    lattice: (37, 37, 37) -> 37 + 37 * 37 + 37 * 1369 = 52059, which aliases
    through % 50656 to 1403 -- NOT through a wrap at res^3 (that would be 1406)."""
    _, P, b = grid("P")
    corners = hn.level_corners(P, b, np.array([[b, b, b]], np.float32))
    idx1, w1, frac1 = corners[1]
    assert idx1[0, 7] == 4096 + 15624 and idx1[0, 0] == 4096 + 23 + 23 * 25 + 23 * 625
    assert abs(float(frac1[0, 0]) - (P[1][0] + 0.5 - 23)) < 1e-5
    idx2, w2, _ = corners[2]
    assert idx2[0, 7] == 19728 + 1403
    assert idx2[0, 1] == 19728 + (37 + 36 * 37 + 36 * 1369) % 50656
    assert w2[0, 7] > 0.01                              # a real contribution, not a zero weight
    idx0, w0, frac0 = corners[0]                        # integer scale: frac = 0.5, corner 16 = res
    assert (frac0 == 0.5).all() and idx0[0, 7] == (16 + 16 * 16 + 16 * 256) % 4096 and w0[0, 7] == 0.125
    # every index of every set is inside its level's slab
    for gname in GRIDS:
        _, levels, _ = grid(gname)
        for sname in SETS:
            for lv, (idx, _, _) in zip(levels, case(gname, sname)[1]):
                assert idx.min() >= lv[3] and idx.max() < lv[3] + lv[2]


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("gname", list(GRIDS))
def test_encode_matches_the_oracle(gname, sname):
    spec, levels, bound = grid(gname)
    x, corners, _, _ = case(gname, sname)
    rng = np.random.default_rng(5)
    table = rng.standard_normal((hn.total_entries(levels), 2)).astype(np.float32)
    feat, mag = hn.encode_from(corners, table)
    x01 = torch.from_numpy(hn.unit_coords(x, bound))
    got = ofield.hashgrid_encode(spec, x01, torch.from_numpy(table).view(-1))
    got = got.view(x.shape[0], len(levels), 2).permute(1, 0, 2).numpy()
    hn.compare_features(got, feat, hn.bound_fwd(mag), f"oracle encode [{gname}-{sname}]")
    # fp16 features: the oracle's rounding of the same values
    got_h = torch.from_numpy(got).half().numpy()
    hn.compare_features(got_h, feat, hn.bound_fwd(mag, feat, True), f"oracle encode, half [{gname}-{sname}]")
    # the oracle's own unit mapping is the kernels'
    ox01 = (torch.from_numpy(x) + bound) / (2 * bound)
    assert torch.equal(ox01, x01)


@pytest.mark.parametrize("sname", SETS)
@pytest.mark.parametrize("gname", list(GRIDS))
def test_grad_matches_oracle_autograd_and_plain_fp32(gname, sname):
    """The reference alone is within the bound: fp32 sequential accumulation of
    the same formula, and the oracle's autograd."""
    spec, levels, bound = grid(gname)
    x, corners, d_feat, ref = case(gname, sname)
    total = hn.total_entries(levels)
    seq = hn.grad_fp32_sequential(corners, d_feat, total)
    r_seq = hn.compare_table(seq, ref, hn.bound_bwd(ref), what=f"fp32 sequential [{gname}-{sname}]")
    params = torch.zeros(total * 2, requires_grad=True)
    enc = ofield.hashgrid_encode(spec, torch.from_numpy(hn.unit_coords(x, bound)), params)
    d_out = torch.from_numpy(d_feat).permute(1, 0, 2).reshape(x.shape[0], -1)
    enc.backward(d_out)
    auto = params.grad.view(-1, 2).numpy()
    r_auto = hn.compare_table(auto, ref, hn.bound_bwd(ref), what=f"oracle autograd [{gname}-{sname}]")
    assert np.array_equal(auto == 0, seq == 0)
    assert 0.0 < r_seq and 0.0 < r_auto                 # fp32 is not float64: the check bites
    # the tighter budgets hold for exact values, as they must
    exact = ref.dense(total)
    assert hn.compare_table(exact, ref, hn.bound_bwd_det(ref)) == 0.0
    assert (hn.bound_bwd_p64(ref, levels) >= hn.bound_bwd(ref)).all()
    assert (hn.bound_bwd_h16(ref, levels, 65536.0) >= hn.bound_bwd(ref)).all()


def test_compare_table_checks_the_whole_table_and_the_prior():
    _, levels, _ = grid("S")
    _, _, _, ref = case("S", "faces")
    total = hn.total_entries(levels)
    good = ref.dense(total)
    hn.compare_table(good, ref, hn.bound_bwd(ref))
    hn.compare_table(good + 1.0, ref, hn.bound_bwd(ref), prior=1.0)
    untouched = np.setdiff1d(np.arange(total), ref.idx)
    assert untouched.size > 0
    bad = good.copy()
    bad[untouched[0], 1] = 1e-30                        # a stray write outside the touched set
    with pytest.raises(AssertionError):
        hn.compare_table(bad, ref, hn.bound_bwd(ref))
    with pytest.raises(AssertionError):                 # overwrote instead of added
        hn.compare_table(good, ref, hn.bound_bwd(ref), prior=1.0)
    bad = good.copy()
    bad[ref.idx[0], 0] = np.nan
    with pytest.raises(AssertionError):
        hn.compare_table(bad, ref, hn.bound_bwd(ref))
    # a sample with d_feat = (0, 0) contributes nothing, not even to n
    _, corners, d_feat, _ = case("S", "faces")
    assert int(ref.n.sum()) == 8 * int(((d_feat != 0).any(2)).sum())


# ---------------------------------------------------------------------------
# sharpness: wrong references, same inputs -> rejected
# ---------------------------------------------------------------------------
def _rejects(levels, corners_bad, d_feat, ref, bound=None):
    bad = hn.grad_from(corners_bad, d_feat).dense(hn.total_entries(levels))
    with pytest.raises(AssertionError):
        hn.compare_table(bad, ref, hn.bound_bwd(ref) if bound is None else bound)
    return bad


def _all_bounds(ref, levels):
    """The widest budget any backward entry point is given."""
    return np.maximum(hn.bound_bwd_p64(ref, levels), hn.bound_bwd_h16(ref, levels, 65536.0))


def test_sharpness_wrap_at_res_cubed_on_dense_levels():
    _, levels, bound = grid("P")
    x, corners, d_feat, ref = case("P", "faces")
    x01 = hn.unit_coords(x, bound)
    bad = list(corners)
    changed = 0
    for l, lv in enumerate(levels):
        if lv[4]:
            continue
        cell, frac = hn.cell_frac(x01, lv[0])
        idx = np.empty((x.shape[0], 8), np.int64)
        for c in range(8):
            g = [cell[:, a] + ((c >> a) & 1) for a in range(3)]
            idx[:, c] = (g[0] + g[1] * lv[1] + g[2] * lv[1] ** 2) % lv[1] ** 3 + lv[3]
        changed += int((idx != corners[l][0]).sum())
        bad[l] = (idx, corners[l][1], frac)
    assert changed > 0
    _rejects(levels, bad, d_feat, ref, _all_bounds(ref, levels))
    # ... and by the forward comparison
    table = np.random.default_rng(5).standard_normal((hn.total_entries(levels), 2)).astype(np.float32)
    feat, mag = hn.encode_from(corners, table)
    feat_bad, _ = hn.encode_from(bad, table)
    with pytest.raises(AssertionError):
        hn.compare_features(feat_bad, feat, hn.bound_fwd(mag, feat, True))


@pytest.mark.parametrize("gname,sname", [("P", "box"), ("P", "faces"), ("S", "faces"), ("D", "box")])
def test_sharpness_one_dropped_corner(gname, sname):
    """One contribution of one sample missing (or counted twice) at an entry
    with n <= 25 or so overshoots every budget by orders of magnitude.  (Not so
    in the one-cell set: one of 3500 contributions to an entry is inside the
    fp32 round-off of a 3500-term sum -- that set is there for runs, overflowing
    bins and contention, where whole groups of contributions go missing.)"""
    _, levels, _ = grid(gname)
    _, corners, d_feat, ref = case(gname, sname)
    l = len(levels) - 2
    m = int(np.flatnonzero((d_feat[l] != 0).any(1))[len(d_feat[l]) // 3])
    idx, w, frac = corners[l]
    c = int(np.argmax(w[m]))
    w2 = w.copy()
    w2[m, c] = 0.0
    bad = list(corners)
    bad[l] = (idx, w2, frac)
    _rejects(levels, bad, d_feat, ref, _all_bounds(ref, levels))
    w2[m, c] = 2.0 * w[m, c]                            # ... or doubled
    _rejects(levels, bad, d_feat, ref, _all_bounds(ref, levels))


def test_sharpness_swapped_hash_primes_on_one_level():
    _, levels, bound = grid("P")
    x, corners, d_feat, ref = case("P", "box")
    l = 4
    cell, frac = hn.cell_frac(hn.unit_coords(x, bound), levels[l][0])
    idx = np.empty((x.shape[0], 8), np.int64)
    for c in range(8):                                  # y and z exchanged = primes exchanged
        idx[:, c] = hn.corner_index(levels[l], cell[:, 0] + (c & 1), cell[:, 2] + ((c >> 2) & 1),
                                    cell[:, 1] + ((c >> 1) & 1))
    bad = list(corners)
    bad[l] = (idx, corners[l][1], frac)
    _rejects(levels, bad, d_feat, ref, _all_bounds(ref, levels))


@pytest.mark.parametrize("gname", ["P", "D"])
def test_sharpness_cells_from_a_float64_position(gname):
    _, levels, bound = grid(gname)
    x, corners, d_feat, ref = case(gname, "box")
    x01 = (x.astype(np.float64) + bound) / (2.0 * bound)
    bad = []
    for lv in levels:
        pos = x01 * lv[0] + 0.5
        cell = np.floor(pos)
        frac = pos - cell
        cell = cell.astype(np.int64)
        idx = np.empty((x.shape[0], 8), np.int64)
        for c in range(8):
            idx[:, c] = hn.corner_index(lv, cell[:, 0] + (c & 1), cell[:, 1] + ((c >> 1) & 1),
                                        cell[:, 2] + ((c >> 2) & 1))
        bad.append((idx, hn.corner_weights(frac), frac))
    _rejects(levels, bad, d_feat, ref)
    table = np.random.default_rng(5).standard_normal((hn.total_entries(levels), 2)).astype(np.float32)
    feat, mag = hn.encode_from(corners, table)
    with pytest.raises(AssertionError):
        hn.compare_features(hn.encode_from(bad, table)[0], feat, hn.bound_fwd(mag))


def test_merged_reference_is_the_sum_of_its_passes_and_rejects_shifted_rows():
    _, levels, bound = grid("S")
    o, d, z_c, z_f, _ = hn.merged_case(bound)
    aabb, L = hn.aabb_of(bound), len(levels)
    d_c = hn.d_feat_for(L, z_c.size, 31)
    d_f = hn.d_feat_for(L, z_f.size, 32)
    ref = hn.grad_merged(levels, bound, o, d, z_c, z_f, aabb, d_c, d_f)
    total = hn.total_entries(levels)
    two = (hn.grad_rays(levels, bound, o, d, z_c, aabb, d_c).dense(total) +
           hn.grad_rays(levels, bound, o, d, z_f, aabb, d_f).dense(total))
    # float64 round-off of two differently ordered n-term sums only
    hn.compare_table(two, ref, (ref.n[:, None] + 2) * 2.0 ** -52 * ref.A)
    bad = hn.grad_merged(levels, bound, o, d, z_c, z_f, aabb, d_c, np.roll(d_f, 1, axis=1))
    with pytest.raises(AssertionError):
        hn.compare_table(bad.dense(total), ref, _all_bounds(ref, levels))
