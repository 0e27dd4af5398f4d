"""Every ``ucsa_hashgrid_encode_*`` and ``ucsa_hashgrid_bwd_*`` entry point
against the float64 reference of tests/hashgrid_numpy.py, element by element,
within budgets derived from the rounding steps of the code (never a flat
number): the production level table (its level 4 is hashed AND below the bin
threshold: the one level where hashed indices go through the run-combining /
LDS-accumulator kernel), a small table whose 4096-entry levels make corners
collide, a table whose bound takes the division branch of the unit mapping;
points on the far faces of the box, tail sizes, one crowded cell, runs across
ray and wave boundaries, zero gradients inside runs.

One test id = one entry point on one input.  Each comparison prints its worst
err / bound (recorded in docs/DESIGN_NOTEBOOK.md).  The sharpness of the
comparison itself is shown on the CPU, tests/test_hashgrid_reference_cpu.py.
"""
import numpy as np
import pytest
import torch

from tests import hashgrid_numpy as hn

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (bound, n_levels, log2_hashmap_size, base_resolution, per_level_scale)
GRID_ARGS = {
    "P": (4.0, 16, 19, 16, float(np.exp2(np.log2(2048 * 4.0 / 16) / 15))),
    "S": (4.0, 8, 12, 16, 2.0),
    "D": (3.0, 8, 12, 16, 2.0),
}
SIZES = (1, 63, 64, 65, 255, 256, 257, 2049)
POINT_SETS = ("faces", "one_cell") + tuple(f"size{m}" for m in SIZES)
REC_SCALE = 65536.0
_cache = {}


def memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as o
    return o


def grid(name):
    """(Grid struct, level rows, bound, total entries)."""
    def make():
        from ucsa_neural_rendering_amd._lib import make_grid
        g = make_grid(*GRID_ARGS[name])
        levels = hn.levels_of(g)
        assert hn.total_entries(levels) == int(g.total_entries)
        return g, levels, float(g.bound), int(g.total_entries)
    return memo(("grid", name), make)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table(name):
    """N(0, 1) table values: (numpy fp32 [total, 2], device tensor)."""
    def make():
        total = grid(name)[3]
        t = np.random.default_rng(17).standard_normal((total, 2)).astype(np.float32)
        return t, cu(t)
    return memo(("table", name), make)


def points(gname, sname):
    _, levels, bound, _ = grid(gname)
    if sname == "faces":
        return hn.points_faces(bound)
    if sname == "one_cell":
        return hn.points_one_cell(levels, bound)
    if sname == "many_cells":
        return hn.points_box(120001, bound, 7)
    return hn.points_box(int(sname[4:]), bound, 100 + int(sname[4:]))


def point_case(gname, sname):
    """(x, corners, d_feat, reference gradient): computed once per module."""
    def make():
        _, levels, bound, _ = grid(gname)
        x = points(gname, sname)
        corners = hn.level_corners(levels, bound, x)
        d_feat = hn.d_feat_for(len(levels), x.shape[0], 21)
        return x, corners, d_feat, hn.grad_from(corners, d_feat)
    return memo(("points", gname, sname), make)


def ray_case(gname, magnitude=1.0, sparse=False):
    def make():
        _, levels, bound, _ = grid(gname)
        o, d, z = hn.sparse_rays_case(bound) if sparse else hn.rays_case(bound)
        corners = hn.level_corners(levels, bound, hn.ray_points(o, d, z, hn.aabb_of(bound)))
        d_feat = hn.d_feat_for(len(levels), z.size, 22, magnitude)
        return o, d, z, corners, d_feat, hn.grad_from(corners, d_feat)
    return memo(("rays", gname, magnitude, sparse), make)


def merged_case(gname, magnitude=1.0, sparse=False):
    def make():
        _, levels, bound, _ = grid(gname)
        if sparse:      # the sparse rays' samples dealt alternately to the two passes
            o, d, z = hn.sparse_rays_case(bound)
            z_c, z_f = np.ascontiguousarray(z[:, 0::2]), np.ascontiguousarray(z[:, 1::2])
            src = np.argsort(np.concatenate([z_c, z_f], 1), axis=1, kind="stable").astype(np.int32)
        else:
            o, d, z_c, z_f, src = hn.merged_case(bound)
        L = len(levels)
        d_c = hn.d_feat_for(L, z_c.size, 31, magnitude)
        d_f = hn.d_feat_for(L, z_f.size, 32, magnitude)
        if not sparse:
            d_f[:, 2::5] = 0.0
        ref = hn.grad_merged(levels, bound, o, d, z_c, z_f, hn.aabb_of(bound), d_c, d_f)
        return o, d, z_c, z_f, src, d_c, d_f, ref
    return memo(("merged", gname, magnitude, sparse), make)


def image_case(gname):
    def make():
        _, levels, bound, _ = grid(gname)
        o, d, z = hn.image_case(bound)
        corners = hn.level_corners(levels, bound, hn.ray_points(o, d, z, hn.aabb_of(bound)))
        return o, d, z, corners
    return memo(("image", gname), make)


def new_table(gname, fill=0.0):
    return torch.full((grid(gname)[3], 2), fill, device=DEV)


def fetch(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------------------
# the tables the cases rely on
# ---------------------------------------------------------------------------
def test_grids_have_the_levels_the_cases_rely_on():
    _, P, _, _ = grid("P")
    assert len(P) == 16 and P[4][4] and P[4][0] < hn.BIN_SCALE      # hashed, not binned
    assert list(hn.binned_levels(P)) == [False] * 5 + [True] * 11
    assert not P[2][4] and P[2][2] != P[2][1] ** 3                # dense, entries != res^3
    _, S, _, _ = grid("S")
    assert [lv[4] for lv in S] == [False] + [True] * 7 and all(lv[2] == 4096 for lv in S)
    assert list(hn.binned_levels(S)) == [False] * 3 + [True] * 5   # two hashed levels unbinned
    assert grid("D")[2] == 3.0
    # the oracle's table is the library's (the CPU tests read the oracle's)
    from oracle.field import make_grid_spec
    assert hn.levels_of(make_grid_spec(4.0)) == P
    assert hn.levels_of(make_grid_spec(4.0, n_levels=8, log2_hashmap_size=12, per_level_scale=2.0)) == S


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def run_bwd_points(ops, gname, sname, binned, prior=0.0, one_add=True):
    g = grid(gname)[0]
    x, _, d_feat, ref = point_case(gname, sname)
    assert d_feat.shape == (g.n_levels, x.shape[0], 2)
    gt = new_table(gname, prior)
    ops.hashgrid_bwd_points(g, cu(x), cu(d_feat), gt, binned=binned)
    if prior != 0.0 and one_add:
        assert int(ref.n.max()) == 1
    return hn.compare_table(fetch(gt), ref, hn.bound_bwd(ref), prior,
                            f"bwd_points binned={binned} [{gname}-{sname}]", one_add)


@pytest.mark.parametrize("binned", [True, False], ids=["binned", "direct"])
@pytest.mark.parametrize("sname", POINT_SETS)
@pytest.mark.parametrize("gname", ["P", "S", "D"])
def test_bwd_points(ops, gname, sname, binned):
    run_bwd_points(ops, gname, sname, binned)


def test_bwd_points_many_cells_binned_P(ops):
    """120 001 points: the multi-tile loop of the run-combining kernel (the host
    picks 2 tiles per workgroup at this size, the last workgroup gets a partial
    one) and its LDS accumulator overflowing into direct atomics on level 4."""
    run_bwd_points(ops, "P", "many_cells", True)


def run_bwd_rays(ops, gname, variant, prior=0.0, zero=False, one_add=True, sparse=False):
    g, levels, bound, _ = grid(gname)
    half = variant == "rec_scale"
    o, d, z, _, d_feat, ref = ray_case(gname, 1e-5 if half else 1.0, sparse)
    if prior != 0.0 and one_add and not zero:
        assert int(ref.n.max()) == 1
    N, T = z.shape
    assert d_feat.shape == (g.n_levels, N * T, 2) and o.shape == d.shape == (N, 3)
    if zero:
        d_feat = np.zeros_like(d_feat)
    if half:    # every record inside the half range (run sums of <= 64 lanes included)
        assert float(np.abs(d_feat).max()) * REC_SCALE * 64 < 65504.0
    gt = new_table(gname, prior)
    kw = dict(binned=dict(binned=True), direct=dict(binned=False), packed=dict(packed=True),
              rec_scale=dict(rec_scale=REC_SCALE))[variant]
    ops.hashgrid_bwd_rays(g, cu(o), cu(d), cu(z), hn.aabb_of(bound), cu(d_feat), gt, **kw)
    got = fetch(gt)
    if zero:
        assert np.count_nonzero(got != prior) == 0
        return 0.0
    b = {"packed": lambda: hn.bound_bwd_p64(ref, levels),
         "rec_scale": lambda: hn.bound_bwd_h16(ref, levels, REC_SCALE)}.get(
             variant, lambda: hn.bound_bwd(ref))()
    return hn.compare_table(got, ref, b, prior, f"bwd_rays {variant} [{gname}]", one_add)


@pytest.mark.parametrize("variant", ["binned", "direct", "packed", "rec_scale"])
@pytest.mark.parametrize("gname", ["P", "S"])
def test_bwd_rays(ops, gname, variant):
    run_bwd_rays(ops, gname, variant)


@pytest.mark.parametrize("variant", ["binned", "packed"])
def test_bwd_rays_all_zero_d_feat_leaves_the_table_untouched(ops, variant):
    run_bwd_rays(ops, "P", variant, prior=1.0, zero=True)


def run_bwd_merged(ops, gname, variant, prior=0.0, one_add=True, sparse=False):
    g, levels, bound, _ = grid(gname)
    half = variant == "rec_scale"
    o, d, z_c, z_f, src, d_c, d_f, ref = merged_case(gname, 1e-5 if half else 1.0, sparse)
    if prior != 0.0 and one_add:
        assert int(ref.n.max()) == 1
    N, Tc, Tf = z_c.shape[0], z_c.shape[1], z_f.shape[1]
    assert d_c.shape == (g.n_levels, N * Tc, 2) and d_f.shape == (g.n_levels, N * Tf, 2)
    assert src.shape == (N, Tc + Tf) and src.min() == 0 and src.max() == Tc + Tf - 1
    gt = new_table(gname, prior)
    kw = dict(plain={}, packed=dict(packed=True), rec_scale=dict(rec_scale=REC_SCALE))[variant]
    ops.hashgrid_bwd_rays_merged(g, cu(o), cu(d), cu(z_c), cu(z_f), cu(src), hn.aabb_of(bound),
                                 cu(d_c), cu(d_f), gt, **kw)
    b = {"packed": lambda: hn.bound_bwd_p64(ref, levels),
         "rec_scale": lambda: hn.bound_bwd_h16(ref, levels, REC_SCALE)}.get(
             variant, lambda: hn.bound_bwd(ref))()
    return hn.compare_table(fetch(gt), ref, b, prior, f"bwd_rays_merged {variant} [{gname}]", one_add)


@pytest.mark.parametrize("variant", ["plain", "packed", "rec_scale"])
@pytest.mark.parametrize("gname", ["P", "S"])
def test_bwd_rays_merged(ops, gname, variant):
    run_bwd_merged(ops, gname, variant)


def run_bwd_det(ops, prior=0.0):
    g, _, bound, _ = grid("P")
    o, d, z, _, d_feat, ref = ray_case("P")
    assert d_feat.shape == (g.n_levels, z.size, 2)
    gt = new_table("P", prior)
    fix = ops.hashgrid_bwd_rays_det(g, cu(o), cu(d), cu(z), hn.aabb_of(bound), cu(d_feat))
    ops.hashgrid_bwd_det_finish(g, fix, gt)
    got = fetch(gt)
    hn.compare_table(got, ref, hn.bound_bwd_det(ref), prior, "bwd_rays_det + det_finish [P]")
    return got


def test_bwd_rays_det_P_and_its_bits_repeat(ops):
    a = run_bwd_det(ops)
    b = run_bwd_det(ops)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("family", ["points", "rays", "merged", "det"])
def test_bwd_adds_to_the_table_it_is_given(ops, family):
    """grad_table starts at 1.0: untouched entries stay exactly 1.0, touched
    ones are 1 + g within bound + u (1 + |g|).  That term is ONE rounding at the
    table's magnitude, so the inputs are ones where the gradient reaches every
    entry in one addition whatever the path: a single point and sparse rays
    (every touched entry has exactly one contribution, asserted), and the
    fixed-point path, whose finish kernel adds each complete sum once."""
    if family == "points":
        run_bwd_points(ops, "P", "size1", True, prior=1.0)
    elif family == "rays":
        run_bwd_rays(ops, "P", "packed", prior=1.0, sparse=True)
    elif family == "merged":
        run_bwd_merged(ops, "P", "plain", prior=1.0, sparse=True)
    else:
        run_bwd_det(ops, prior=1.0)


@pytest.mark.parametrize("family", ["points", "rays", "merged"])
def test_bwd_adds_to_the_table_with_many_contributions_per_entry(ops, family):
    """The same on the full-size inputs.  Here an entry is added to more than
    once (workgroups flush their LDS sums with float atomics, overflowing records
    go to the table one by one), each addition rounding at the table's magnitude:
    the faces set through the binned points call sits at 1.66 x the one-addition
    budget for that reason.  Untouched entries stay exactly 1.0; touched ones
    within bound + n u (1 + A)."""
    if family == "points":
        run_bwd_points(ops, "P", "faces", True, prior=1.0, one_add=False)
    elif family == "rays":
        run_bwd_rays(ops, "P", "packed", prior=1.0, one_add=False)
    else:
        run_bwd_merged(ops, "P", "plain", prior=1.0, one_add=False)


def test_bwd_rays_binned_with_a_dirty_oversized_workspace(ops):
    """The cached bin workspace only grows: size it with a larger call, fill it
    with 0xFF (NaN values, entry indices of 4 G), then a small call must read
    nothing it did not write -- checked against the reference."""
    run_bwd_points(ops, "P", "size2049", True)           # (at least) this large
    assert ops._bwd_ws
    for ws in ops._bwd_ws.values():
        ws.fill_(0xFF)
    run_bwd_rays(ops, "P", "binned")
    for ws in ops._bwd_ws.values():
        ws.fill_(0xFF)
    run_bwd_merged(ops, "S", "packed")


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def check_feat(got, corners, tab, what, half_features=False, order=None):
    L, M = len(corners), corners[0][0].shape[0]
    assert tuple(got.shape) == (L, M, 2)
    assert got.dtype == (torch.float16 if half_features else torch.float32)
    feat, mag = hn.encode_from(corners, tab)
    if order is not None:
        feat, mag = feat[:, order], mag[:, order]
    return hn.compare_features(fetch(got), feat, hn.bound_fwd(mag, feat, half_features), what)


def half_table(ops, gname):
    """(fp16-rounded values as numpy, the table-to-half op's device tensor)."""
    def make():
        t, t_dev = table(gname)
        th = ops.table_to_half(t_dev)
        ref = t.astype(np.float16)
        assert th.dtype == torch.float16 and th.numel() == t.size
        assert np.array_equal(fetch(th).view(np.uint16), ref.reshape(-1).view(np.uint16))
        return ref, th
    return memo(("half", gname), make)


@pytest.mark.parametrize("sname", ("faces",) + tuple(f"size{m}" for m in SIZES))
@pytest.mark.parametrize("gname", ["P", "S", "D"])
def test_encode_points(ops, gname, sname):
    g = grid(gname)[0]
    x, corners, _, _ = point_case(gname, sname)
    t, t_dev = table(gname)
    got = ops.hashgrid_encode_points(g, t_dev, cu(x))
    check_feat(got, corners, t, f"encode_points [{gname}-{sname}]")


@pytest.mark.parametrize("form", ["plain", "half_features", "half_table"])
@pytest.mark.parametrize("gname", ["P", "S"])
def test_encode_rays(ops, gname, form):
    g, _, bound, _ = grid(gname)
    o, d, z, corners, _, _ = ray_case(gname)
    t, t_dev = table(gname)
    if form == "half_table":
        t, t_dev = half_table(ops, gname)
    got = ops.hashgrid_encode_rays(g, t_dev, cu(o), cu(d), cu(z), hn.aabb_of(bound),
                                   half_features=form == "half_features")
    check_feat(got, corners, t, f"encode_rays {form} [{gname}]", form != "plain")


@pytest.mark.parametrize("form", ["image", "image_half_features", "image_half_table",
                                  "sorted", "sorted_half_features"])
@pytest.mark.parametrize("gname", ["P", "S"])
def test_encode_image_order(ops, gname, form):
    """Rays as the pixels of a 16 x 24 image: the tiled kernels, and the
    depth-ordered ones (results mapped back through ``slot``)."""
    g, _, bound, _ = grid(gname)
    o, d, z, corners = image_case(gname)
    N, T = z.shape
    W = 24
    assert N % W == 0
    t, t_dev = table(gname)
    aabb = hn.aabb_of(bound)
    half = form.endswith("half_features") or form == "image_half_table"
    order = None
    if form.startswith("sorted"):
        z_dev = cu(z)
        zs, pix, slot = ops.tile_depth_order(z_dev, W)
        order = fetch(slot).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(N * T))
        assert np.array_equal(fetch(zs), z.reshape(-1)[order])
        got = ops.hashgrid_encode_sorted(g, t_dev, cu(o), cu(d), zs, pix, aabb, T, W,
                                         half_features=half)
    else:
        if form == "image_half_table":
            t, t_dev = half_table(ops, gname)
        got = ops.hashgrid_encode_rays(g, t_dev, cu(o), cu(d), cu(z), aabb, image_width=W,
                                       half_features=form == "image_half_features")
    check_feat(got, corners, t, f"encode_rays {form} [{gname}]", half, order)
