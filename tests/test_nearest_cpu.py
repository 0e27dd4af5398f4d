"""CPU: the nearest-point contract (tests/nearest_numpy.py).  The model of the
kernel's traversal, ``nearest_point_grid`` (cells, rings, stop rule), equals the
brute-force definition ``nearest_point`` byte for byte on every input the GPU
test uses, for every cell size and for a moved origin; hand cases with the
expected arrays written out pin the inclusive radius and the tie rule."""
import numpy as np
import pytest

from tests import nearest_numpy as NN

F = np.float32
# 0.25 and 0.5 put the lattice's points on cell walls (one and two lattice planes
# per cell), 0.3 and 0.37 have walls between them, 4.0 is a single cell
CELLS = [None, 0.05, 0.25, 0.3, 0.37, 0.5, 4.0]


def lattice_case():
    """A 9 x 7 x 5 lattice scaled by 0.25, shuffled so that index order differs
    from cell order; queries at edge, face and body midpoints: exact 2-, 4- and
    8-way ties (every coordinate is a multiple of 1/8, every d2 exact)."""
    g = np.random.default_rng(5)
    ijk = np.stack(np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing="ij"), -1)
    ijk = ijk.reshape(-1, 3)
    pts = (ijk[g.permutation(ijk.shape[0])] * 0.25).astype(F)
    q = []
    for half in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
        h = np.asarray(half)
        base = ijk[((ijk + h) < np.array([9, 7, 5])).all(1)]
        q.append((base + 0.5 * h) * 0.25)
    q = np.concatenate(q).astype(F)
    return pts, q[g.permutation(q.shape[0])], 0.25


def duplicates_case():
    """every position four times under different indices, as the shared borders
    of the room mesh's rectangles are; queries on and off the points"""
    g = np.random.default_rng(6)
    base = g.random((150, 3)).astype(F)
    pts = np.concatenate([base, base[::-1], base, base[g.permutation(150)]])
    q = np.concatenate([base[:40], g.random((60, 3)).astype(F)])
    return pts, q, 0.3


def sparse_case():
    """3000 points in the unit cube, outliers at +-50 (a mostly empty grid), a NaN
    and an inf point; 2000 queries: inside the cube, outside the points' box by
    0.005, 0.1, 150 and 300 (less and more than each max_dist of MAX_DISTS), one
    NaN and one inf query.

    The box is 100 wide, so every cell of CELLS below 4.0 is raised to about 2
    here (the grid's cap of 64 cells per point, and 2^24 cells whatever the
    cap): the unit cube sits in one to eight cells and this case tests the far
    walks, the empty cells and the non-finite values, not the pruning among the
    cube's own points.  ``sparse_near_case`` does that on a sparse grid whose
    small cells survive."""
    g = np.random.default_rng(7)
    pts = g.random((3004, 3)).astype(F)
    pts[100] = 50.0
    pts[2000] = -50.0
    pts[7] = (0.5, np.nan, 0.5)
    pts[3001] = (np.inf, 0.5, 0.5)
    q = g.random((2000, 3)).astype(F)
    k = 1962                                                       # few walk far: seconds here
    for out in (0.005, 0.1, 150.0, 300.0):
        for _ in range(6):
            p = (g.random(3) * 100 - 50)
            ax = int(g.integers(0, 3))
            p[ax] = (50 + out) * (1 if g.random() < 0.5 else -1)
            q[k] = p
            k += 1
    q[k:1998, :] = g.random((1998 - k, 3)) * 100 - 50             # inside the box, off the cube
    q[1996] = (50.004, 50.0, 50.0)                                # next to an outlier
    q[1997] = (-50.0, -50.1, -50.0)
    q[1998] = (0.5, 0.5, np.nan)
    q[1999] = (-np.inf, 0.5, 0.5)
    return pts, q


def sparse_near_case():
    """The sparse case's points with the outliers at +-1.5 instead of +-50: a box 3
    wide, of which the unit cube is 1/27.  Cells 0.25, 0.3, 0.37 and 0.5 stay as
    asked and 0.05 is raised to 0.0625 only, so the cube spans 2 to 16 cells a
    side and the cuts act among its own points on a mostly empty grid.  700
    queries: in the cube, in the box off the cube, outside the box by 0.005, 0.1
    and 1 (max_dist 0.2), a NaN and an inf query."""
    pts, _ = sparse_case()
    pts = pts.copy()
    pts[100] = 1.5
    pts[2000] = -1.5
    g = np.random.default_rng(9)
    q = g.random((700, 3)).astype(F)
    q[500:680] = (g.random((180, 3)) * 3 - 1.5).astype(F)
    k = 680
    for out in (0.005, 0.1, 1.0):
        for _ in range(6):
            p = g.random(3) * 3 - 1.5
            p[int(g.integers(0, 3))] = (1.5 + out) * (1 if g.random() < 0.5 else -1)
            q[k] = p
            k += 1
    q[698] = (0.5, np.nan, 0.5)
    q[699] = (0.5, 0.5, np.inf)
    return pts, q, 0.2


MAX_DISTS = [0.01, 0.2, 200.0]


def sized_cases():
    """name -> (points, queries, max_dist): the degenerate sizes"""
    g = np.random.default_rng(8)
    pts = g.random((200, 3)).astype(F)
    return {"n1_q1": (pts[:1], pts[:1] + F(0.01), 0.1),
            "n0": (pts[:0], pts[:5], 0.1),
            "q0": (pts, pts[:0], 0.1),
            "q65": (pts, g.random((65, 3)).astype(F), 0.15),
            "q129": (pts, g.random((129, 3)).astype(F), 0.15)}


def all_cases():
    out = dict(sized_cases())
    out["lattice"] = lattice_case()
    p, q, md = lattice_case()
    out["lattice_wide"] = (p, q, 0.6)
    out["duplicates"] = duplicates_case()
    p, q = sparse_case()
    for md in MAX_DISTS:
        out[f"sparse_{md}"] = (p, q, md)
    out["sparse_near"] = sparse_near_case()
    return out


_WANT = {}


def want(name):
    """the definition's answer, computed once and shared (read-only)"""
    if name not in _WANT:
        p, q, md = all_cases()[name]
        idx, d2 = NN.nearest_point(p, q, md)
        idx.setflags(write=False)
        d2.setflags(write=False)
        _WANT[name] = (idx, d2)
    return _WANT[name]


def same(got, ref):
    return (got[0].dtype == np.int32 and got[1].dtype == F and
            got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes())


@pytest.mark.parametrize("name", sorted(all_cases()))
def test_grid_model_equals_brute_force_for_every_cell_size(name):
    p, q, md = all_cases()[name]
    ref = want(name)
    for cell in CELLS:
        assert same(NN.nearest_point_grid(p, q, md, cell=cell), ref), (name, cell)
    # a moved origin, and queries in another order
    assert same(NN.nearest_point_grid(p, q, md, cell=0.3, origin=(-0.77, -0.31, -1.9)), ref)
    perm = np.random.default_rng(1).permutation(q.shape[0])
    got = NN.nearest_point_grid(p, q[perm], md, cell=0.37)
    assert got[0].tobytes() == ref[0][perm].tobytes() and got[1].tobytes() == ref[1][perm].tobytes()


def test_the_cases_hold_what_they_are_for():
    p, q, md = lattice_case()
    idx, d2 = want("lattice")
    assert (idx >= 0).all()
    # 2-, 4- and 8-way ties at d2 = 1, 2 and 3 times (1/8)^2, and the smallest index won
    with np.errstate(all="ignore"):
        dd = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    ways = (dd == d2[:, None]).sum(1)
    assert sorted(np.unique(ways).tolist()) == [2, 4, 8]
    assert (idx == np.argmax(dd == d2[:, None], axis=1)).all()
    assert not (np.diff(NN.point_grid(p, 0.25)["order"]) > 0).all()       # shuffled
    # the sparse grid is mostly empty, and the pruning visits a small part of it
    p, q = sparse_case()
    st = {}
    NN.nearest_point_grid(p, q[:1962], 0.2, cell=0.05, stats=st)
    g = NN.point_grid(p, 0.05)
    assert (np.diff(g["offsets"]) == 0).mean() > 0.9 and g["offsets"][-1] == 3002
    assert st["cells_visited"] < 1962 * 200 < 1962 * st["cells"] // 100
    for md in MAX_DISTS:
        idx, _ = want(f"sparse_{md}")
        assert idx[1998] == -1 and idx[1999] == -1 and 7 not in idx and 3001 not in idx
        assert (idx[:1962] >= 0).any() and (idx[1962:1986] == -1).any()
    assert (want("sparse_200.0")[0][1962:1980] >= 0).all()         # outside by less than 200
    assert (want("sparse_200.0")[0][1980:1986] == -1).all()        # by more
    assert (want("sparse_0.2")[0][1962:1974] >= 0).sum() < 12      # 0.005 and 0.1 outside
    assert want("sparse_0.01")[0][1996] == 100 and want("sparse_0.2")[0][1997] == 2000
    # the wide box raises every small cell, the near one keeps them
    assert all(NN.point_grid(p, c)["cell"] > 1.5 for c in (0.05, 0.25, 0.3, 0.37, 0.5))
    p, q, md = sparse_near_case()
    assert [float(NN.point_grid(p, c)["cell"]) for c in (0.25, 0.3, 0.37, 0.5)] == \
        [float(F(c)) for c in (0.25, 0.3, 0.37, 0.5)]
    g = NN.point_grid(p, 0.05)
    assert g["cell"] < 0.07 and (np.diff(g["offsets"]) == 0).mean() > 0.9
    st = {}
    NN.nearest_point_grid(p, q[:500], md, cell=0.05, stats=st)
    assert st["cells_visited"] < 500 * 400 < 500 * st["cells"] // 100
    idx, _ = want("sparse_near")
    assert (idx[:500] >= 0).all() and (idx[680:692] >= 0).sum() < 12 and (idx[692:] == -1).all()


def test_hand_cases_radius_is_inclusive_and_smaller_index_wins():
    one = np.zeros((1, 3), F)
    at = np.array([[0.5, 0, 0]], F)
    for fn in (NN.nearest_point, NN.nearest_point_grid):
        idx, d2 = fn(one, at, 0.5)
        assert idx.tolist() == [0] and d2.tolist() == [0.25]
        idx, d2 = fn(one, np.array([[np.nextafter(F(0.5), F(1)), 0, 0]], F), 0.5)
        assert idx.tolist() == [-1] and d2.tolist() == [np.inf]
        # equidistant points: index order against cell order, both ways round
        a, b = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]
        mid = np.array([[0.5, 0, 0], [0.5, 0.25, 0], [0.25, 0, 0]], F)
        for pts in ([a, b], [b, a]):
            idx, d2 = fn(np.array(pts, F), mid, 1.0)
            assert idx.tolist() == [0, 0, pts.index(a)]
            assert d2.tolist() == [0.25, 0.3125, 0.0625]
    for cell in CELLS:
        idx, d2 = NN.nearest_point_grid(np.array([b, a], F), mid, 1.0, cell=cell)
        assert idx.tolist() == [0, 0, 1] and d2.tolist() == [0.25, 0.3125, 0.0625]
    with pytest.raises(ValueError):
        NN.nearest_point(one, at, 0.0)
    with pytest.raises(ValueError):
        NN.nearest_point(one, at, float("inf"))
    with pytest.raises(ValueError):
        NN.nearest_point_grid(one, at, 1e30)


def test_cell_keys_clamp_and_sort_key():
    o, dims = np.zeros(3, F), (4, 3, 2)
    x = np.array([[0, 0, 0], [0.99, 0.74, 0.49], [-5, 0.3, 0.3], [0.3, 9, 0.3], [np.nan, 0, 0],
                  [0, np.inf, 0], [3e38, 3e38, 3e38], [0.25, 0.25, 0.25]], F)
    assert NN.cell_keys(x, o, F(0.25), dims).tolist() == [0, 23, 3, 11, 24, 24, 23, 9]
    assert NN.cell_keys(x, o, F(0.25), dims, clamp=False).tolist() == [0, 23, 24, 24, 24, 24, 24, 9]
