"""CPU: the properties of the mesh surface sampling contract as
tests/sample_numpy.py restates it (no GPU): exact weights, points on their
faces within a derived rounding allowance, the prefix and independence
properties, no samples on invalid or empty faces, the count's stochastic
rounding, and the uniformity of the point set on one triangle.  The cases and
their expected outputs are shared with tests/test_gpu_sample.py, which holds
the kernels to them byte for byte.

The allowance of a point's distance to its face.  u = 2^-24 is float32's unit
roundoff, E the face's largest edge component, L its largest corner coordinate.
Per axis the sample is A + (w1*e1 + w2*e2) with w1 + w2 <= 1: the two edges and
the two products round by at most u*E each, weighted by w1 and w2 (2uE in all),
the sum by uE, the last addition by uL: u(3E + L).  The distance is measured by
surface_numpy.closest in float32: the corners minus the query (magnitude <= E,
uE), seven and a half roundings of that magnitude on the way to the closest
point (docs/DESIGN_NOTEBOOK.md, section NT), and the weights it finds, whose
determinants are sums of products of E^4 divided by (2 area)^2: a relative
2^-24 there moves the point by u*E*k with k = max(1, len^4 / (4 area^2)), len
the longest edge.  Twelve roundings of size u*E*k and one of u*L per axis,
times sqrt(3) for the three axes."""
import numpy as np
import pytest

from tests import sample_numpy as SP
from tests import surface_numpy as SN
from tests.test_surface_cpu import room, soup

F = np.float32
ONE = SP.ONE
ATTRS = ("normals", "rgb", "labels")


def attributes(g, n):
    nrm = g.normal(size=(n, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F)
    return {"normals": nrm.astype(F), "rgb": g.integers(0, 256, (n, 3)).astype(np.uint8),
            "labels": g.integers(0, 256, n).astype(np.int32)}


def count_of(verts, faces, density, seed):
    return int(SP.face_sample_counts(verts, faces, density, seed)[1].sum())


def density_for(verts, faces, n, seed=0):
    """a density at which the mesh gets ``n`` samples in all: the smallest of a
    bisection's, the total being monotone in the density"""
    lo, hi = 1e-3, 1.0
    while count_of(verts, faces, hi, seed) < n:
        hi *= 2.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if count_of(verts, faces, mid, seed) < n:
            lo = mid
        else:
            hi = mid
    d = float(F(hi * (1.0 + 1e-6)))
    assert count_of(verts, faces, d, seed) == n, (n, d)
    return d


ONE_FACE = (np.array([[0.25, 0.5, -1.0], [1.5, 0.75, -0.5], [0.5, 2.0, 0.25]], F),
            np.array([[0, 1, 2]], np.int32))


def random_case():
    g = np.random.default_rng(31)
    v, f = soup(g, 60, 0.3)
    return dict(verts=v, faces=f, density=600.0, seed=7, **attributes(g, v.shape[0]))


def zeros_case():
    """runs of faces without a sample between sampled ones: tiny faces (expect
    1e-3), faces of no area, and faces that are not valid"""
    g = np.random.default_rng(32)
    v, f = soup(g, 90, 0.25)
    v = v.reshape(-1, 3, 3)
    for i in range(90):
        kind = (i // 5) % 3
        if kind == 1:
            v[i, 1:] = v[i, :1] + (v[i, 1:] - v[i, :1]) * F(0.004)      # area * 1.6e-5
        elif kind == 2 and i % 2:
            v[i, 2] = v[i, 1]                                           # no area
    v = v.reshape(-1, 3)
    f = f.copy()
    f[[25, 26, 58]] = [[0, 1, 270], [-1, 4, 5], [3, 2 ** 31 - 1, 5]]
    return dict(verts=v, faces=f, density=300.0, seed=3, **attributes(g, v.shape[0]))


def invalid_case():
    g = np.random.default_rng(33)
    v, f = soup(g, 40, 0.3)
    v[7] = (np.nan, 0.5, 0.5)
    v[40] = (0.5, np.inf, 0.5)
    v[80] = (0.5, 0.5, -np.inf)
    v[90:93] = [[3e38, 0, 0], [-3e38, 3e38, 0], [0, -3e38, 3e38]]        # the area overflows
    f = f.copy()
    f[10] = (0, 1, 120)                                                 # V, one past the end
    f[11] = (-1, 4, 5)
    f[12] = (2 ** 31 - 1, 4, 5)
    f[13] = (-2 ** 31, 4, 5)
    return dict(verts=v, faces=f, density=500.0, seed=0xFFFFFFFF, **attributes(g, v.shape[0]))


def room_case():
    c = room()["coarse"]
    g = np.random.default_rng(34)
    a = attributes(g, c["verts"].shape[0])
    a["labels"] = np.asarray(c["labels"]).astype(np.int32)
    return dict(verts=c["verts"].astype(F), faces=c["faces"].astype(np.int32), density=40.0,
                seed=0, **a)


_CASES = {}


def all_cases():
    """name -> dict(verts, faces, density, seed, normals, rgb, labels): shared,
    do not write"""
    if not _CASES:
        r = random_case()
        _CASES["random"] = r
        _CASES["shifted"] = dict(r, verts=(r["verts"] + F(1e4)).astype(F), seed=8)
        _CASES["zeros"] = zeros_case()
        _CASES["invalid"] = invalid_case()
        _CASES["room"] = room_case()
        g = np.random.default_rng(35)
        a1 = attributes(g, 3)
        for n in (0, 1, 65, 5000):
            _CASES[f"one_{n}"] = dict(verts=ONE_FACE[0], faces=ONE_FACE[1], seed=n + 1,
                                      density=density_for(*ONE_FACE, n, n + 1), **a1)
        v, f = soup(g, 9, 0.4)
        _CASES["s257"] = dict(verts=v, faces=f, seed=5, density=density_for(v, f, 257, 5),
                              **attributes(g, 27))
        _CASES["f0"] = dict(r, faces=r["faces"][:0])
        _CASES["v0"] = dict(verts=r["verts"][:0], faces=r["faces"][:4], density=10.0, seed=0,
                            **attributes(g, 0))
    return _CASES


NAMES = ["random", "shifted", "zeros", "invalid", "room", "one_0", "one_1", "one_65", "one_5000",
         "s257", "f0", "v0"]
_WANT = {}


def want(name):
    """the restatement's answer with every attribute, computed once and shared
    (read-only)"""
    if name not in _WANT:
        c = all_cases()[name]
        out = SP.sample_mesh_surface(c["verts"], c["faces"], c["density"], c["seed"],
                                     **{k: c[k] for k in ATTRS})
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WANT[name] = out
    return _WANT[name]


def test_the_cases_hold_what_they_are_for():
    n = {k: want(k)["n_samples"] for k in NAMES}
    print("samples per case:", n)
    assert [n[f"one_{k}"] for k in (0, 1, 65, 5000)] == [0, 1, 65, 5000]
    assert n["s257"] == 257 and n["f0"] == 0 and n["v0"] == 0
    assert (want("s257")["count"] > 0).sum() > 1
    z = want("zeros")["count"]
    runs = np.diff(np.nonzero(z > 0)[0])
    assert runs.max() >= 6 and z[0] > 0 and (z == 0).sum() >= 30
    assert all(300 <= n[k] <= 12000 for k in ("random", "shifted", "zeros", "invalid", "room"))
    for k in NAMES:
        w = want(k)
        assert w["first"].dtype == np.int32 and w["first"][0] == 0
        assert np.array_equal(np.diff(w["first"]), w["count"]) and w["first"][-1] == n[k]


@pytest.mark.parametrize("name", NAMES)
def test_weights_are_exact_and_the_search_finds_the_face(name):
    w = want(name)
    b = w["bary"].astype(np.float64)
    assert (b >= 0).all() and (b.sum(1) == 1.0).all()
    k = b * ONE
    assert (k == np.floor(k)).all()                                  # multiples of 2^-24
    s32 = (w["bary"][:, 0] + w["bary"][:, 1]) + w["bary"][:, 2]
    assert s32.dtype == F and (s32 == F(1)).all()                    # in float32 as well
    # the bounded search gives the definition: face f owns rows first[f] .. first[f+1]
    direct = np.repeat(np.arange(w["count"].size, dtype=np.int32), w["count"])
    assert np.array_equal(w["face"], direct)


def allowance(tri):
    t = tri.astype(np.float64)
    edges = np.stack([t[1] - t[0], t[2] - t[0], t[2] - t[1]])
    E, L = np.abs(edges).max(), np.abs(t).max()
    area2 = np.linalg.norm(np.cross(edges[0], edges[1]))            # twice the area
    k = max(1.0, np.linalg.norm(edges, axis=1).max() ** 4 / area2 ** 2)
    return np.sqrt(3.0) * 2.0 ** -24 * (12.0 * E * k + L)


@pytest.mark.parametrize("name", ["random", "shifted", "room", "one_5000", "s257"])
def test_every_point_lies_on_its_face_within_the_rounding_allowance(name):
    c, w = all_cases()[name], want(name)
    worst = 0.0
    for f in np.nonzero(w["count"])[0]:
        tri = c["verts"][c["faces"][f]]
        p = w["points"][w["first"][f]:w["first"][f + 1]]
        a, b, cc = (tuple((tri[k, x] - p[:, x]).astype(F) for x in range(3)) for k in range(3))
        d = np.sqrt(SN.closest(a, b, cc)[2].astype(np.float64))
        lim = allowance(tri)
        worst = max(worst, float((d / lim).max()))
        assert (d <= lim).all(), (name, f, d.max(), lim)
    print(name, "largest distance / allowance:", worst)
    assert np.isfinite(w["points"]).all()


def test_a_higher_density_appends_and_another_face_changes_nothing():
    c = all_cases()["random"]
    lo = want("random")
    hi = SP.sample_mesh_surface(c["verts"], c["faces"], 2.5 * c["density"], c["seed"],
                                **{k: c[k] for k in ATTRS})
    assert (hi["count"] >= lo["count"]).all() and hi["n_samples"] > 2 * lo["n_samples"]
    for f in range(c["faces"].shape[0]):
        n = int(lo["count"][f])
        a, b = int(lo["first"][f]), int(hi["first"][f])
        for k in ("points", "bary") + ATTRS:
            assert lo[k][a:a + n].tobytes() == hi[k][b:b + n].tobytes(), (f, k)
    # move, shrink and relabel face 20, turn face 21 invalid: every other face keeps its samples
    v, fc = c["verts"].copy(), c["faces"].copy()
    v[fc[20]] = (v[fc[20]] * F(0.5) + F(3.0)).astype(F)
    fc[21] = (0, 1, -1)
    lab = c["labels"].copy()
    lab[fc[20]] = (lab[fc[20]] + 1) % 256
    ed = SP.sample_mesh_surface(v, fc, c["density"], c["seed"], normals=c["normals"], rgb=c["rgb"],
                                labels=lab)
    assert ed["count"][21] == 0 and ed["count"][20] < lo["count"][20]
    for f in range(fc.shape[0]):
        if f in (20, 21):
            continue
        assert ed["count"][f] == lo["count"][f] and ed["area"][f] == lo["area"][f]
        a, b, n = int(lo["first"][f]), int(ed["first"][f]), int(lo["count"][f])
        for k in ("points", "bary") + ATTRS:
            assert lo[k][a:a + n].tobytes() == ed[k][b:b + n].tobytes(), (f, k)


def test_invalid_and_empty_faces_get_no_sample_and_seeds_differ():
    c, w = all_cases()["invalid"], want("invalid")
    bad = [10, 11, 12, 13] + [7 // 3, 40 // 3, 80 // 3, 30]
    assert (w["count"][bad] == 0).all() and (w["area"][bad] == 0).all()
    good = np.setdiff1d(np.arange(40), bad)
    assert (w["area"][good] > 0).all() and np.isfinite(w["points"]).all()
    assert not np.isin(w["face"], bad).any()
    z = want("zeros")
    zc = all_cases()["zeros"]
    flat = [i for i in range(90) if (i // 5) % 3 == 2 and i % 2 and i not in (25, 26, 58)]
    assert (z["area"][flat] == 0).all() and (z["count"][flat] == 0).all()
    assert (z["count"][[25, 26, 58]] == 0).all()
    # the attributes: labels of a corner of the face, colours within the corners' range
    tri = zc["faces"][z["face"]]
    assert (z["labels"][:, None] == zc["labels"][tri]).any(1).all()
    corner = np.argmax(z["bary"], axis=1)                             # the first maximum
    assert np.array_equal(z["labels"], zc["labels"][tri[np.arange(tri.shape[0]), corner]])
    col = zc["rgb"][tri].astype(np.int32)
    assert (z["rgb"] >= col.min(1)).all() and (z["rgb"] <= col.max(1)).all()
    ln = np.linalg.norm(z["normals"].astype(np.float64), axis=1)
    assert (np.abs(ln - 1.0) <= 4 * 2.0 ** -24).all()
    # another seed: another set, of about the same size
    c = all_cases()["random"]
    a, b = want("random"), SP.sample_mesh_surface(c["verts"], c["faces"], c["density"], 8)
    assert a["count"].tobytes() != b["count"].tobytes()
    n = min(a["n_samples"], b["n_samples"])
    assert (a["bary"][:n] != b["bary"][:n]).any(1).mean() > 0.99
    one = SP.sample_mesh_surface(*ONE_FACE, 2000.0, 1)["bary"]
    two = SP.sample_mesh_surface(*ONE_FACE, 2000.0, 2)["bary"]
    assert not set(map(bytes, one)) & set(map(bytes, two))
    for bad_density in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50):
        with pytest.raises(ValueError):
            SP.face_sample_counts(*ONE_FACE, bad_density)
    with pytest.raises(ValueError, match="lower density"):
        SP.sample_mesh_surface(*ONE_FACE, 2000.0, max_samples=100)
    # a huge expectation is clamped to 2^24 per face
    assert SP.face_sample_counts(*ONE_FACE, 1e30)[1][0] == ONE


@pytest.mark.parametrize("nf", [100, 10000])
def test_the_total_is_within_five_deviations_of_the_expectation(nf):
    """count = floor(expect + U), U uniform: unbiased with a variance of at most
    1/4 per face, so the total's deviation is at most sqrt(F) / 2"""
    g = np.random.default_rng(36)
    v, f = soup(g, nf, 0.2)
    worst = 0.0
    for seed in range(20 if nf == 100 else 3):
        area, count, expect = SP.face_sample_counts(v, f, 150.0, seed)
        diff = abs(int(count.sum(dtype=np.int64)) - float(expect.sum(dtype=np.float64)))
        worst = max(worst, diff)
        assert diff <= 2.5 * np.sqrt(nf), (seed, diff)
        assert (np.abs(count - expect.astype(np.float64)) < 1.0 + 1e-6 * expect).all()
    print("F =", nf, "largest |S - sum expect|:", worst, "bound:", 2.5 * np.sqrt(nf))
    assert (count == 0).any() and (count > 1).any()


def _split(c, a, b, unit):
    """the midpoint sub-triangle (0, 1, 2: at that corner; 3: the middle) of the
    integer weights (of ``unit``) and the weights inside it (of ``unit``)"""
    w = np.stack([c, a, b], 1)
    big = 2 * w > unit
    which = np.where(big.any(1), np.argmax(big, 1), 3)
    inner = np.where((which == 3)[:, None], unit - 2 * w, 2 * w)
    rows = np.arange(w.shape[0])
    corner = which < 3
    inner[rows[corner], which[corner]] -= unit
    return which, inner


def test_uniformity_on_one_triangle():
    """N = 4096 points of one face: each of the 4 midpoint sub-triangles holds
    N/4 +- 32, each of their 16 sub-triangles N/16 +- 24 (the issue's bounds; a
    binomial sampler's five deviations would be 139 and 77)"""
    N = 4096
    worst4 = worst16 = 0
    for seed in range(20):
        for f in range(10):
            w = np.asarray([SP.weights(seed, f, j) for j in range(N)], np.int64)
            which, inner = _split(w[:, 0], w[:, 1], w[:, 2], ONE)
            assert (inner >= 0).all() and (inner.sum(1) == ONE).all()
            n4 = np.bincount(which, minlength=4)
            sub, _ = _split(inner[:, 0], inner[:, 1], inner[:, 2], ONE)
            n16 = np.bincount(4 * which + sub, minlength=16)
            worst4 = max(worst4, int(np.abs(n4 - N // 4).max()))
            worst16 = max(worst16, int(np.abs(n16 - N // 16).max()))
            assert np.abs(n4 - N // 4).max() <= 32, (seed, f, n4)
            assert np.abs(n16 - N // 16).max() <= 24, (seed, f, n16)
    print("largest deviation from N/4:", worst4, "from N/16:", worst16)
