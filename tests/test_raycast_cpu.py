"""CPU: the ray-cast contract (tests/raycast_numpy.py).  The model of the
kernel's traversal, ``raycast_grid`` (a slab supercover over the triangle
grid's layers along the ray's major axis, with its slack and its stop rule),
equals the brute-force definition ``raycast_mesh`` byte for byte (face, t, bary
and the any-hit byte) on the meshes of tests/test_surface_cpu.py, at three cell
sizes and for a moved origin: this is the proof of the traversal.  Then
watertightness, an independent float64 cast, the analytic room and hand cases."""
import numpy as np
import pytest

from tests import raycast_numpy as RN
from tests import surface_numpy as SN
from tests.test_surface_cpu import all_cases, cells_of, room

F = np.float32
U = 2.0 ** -24
NAMES = ["random", "shifted", "degenerate", "spanning", "shared", "nonfinite", "flat", "f0", "v0",
         "room"]
INTERIOR = slice(80, 120)        # the rays of ``rays_of`` aimed at interior points


def _box(v):
    fin = v[np.isfinite(v).all(1)] if v.size else v
    if fin.shape[0] == 0:
        return np.zeros(3, F), np.ones(3, F)
    return fin.min(0), fin.max(0)


_RAYS, _WANT = {}, {}


def rays_of(name):
    """-> (origins, dirs, t_min, t_max), float32, about 160 rays: origins inside
    and outside the box; 40 each aimed at face corners, edge midpoints and
    interior points, 28 at random points; axis-aligned rays; rays in the plane
    z = 0.5 (the plane of ``flat``) and across it; a non-finite ray and a zero
    direction; a whole line (t_min = -inf); finite t_max just short of, at and
    just beyond a hit.  Shared and read-only."""
    if name in _RAYS:
        return _RAYS[name]
    v, f, _, _ = all_cases()[name]
    g = np.random.default_rng(100 + NAMES.index(name))
    lo, hi = _box(v)
    ext = np.maximum(hi - lo, F(1e-3))
    n = 148
    o = (lo + g.random((n, 3)) * ext).astype(F)
    out = np.arange(n) % 2 == 1
    side = np.where(g.random((n, 3)) < 0.5, -1.0, 1.0)
    o[out] = (o[out] + (side * (0.5 + g.random((n, 3))) * ext)[out]).astype(F)
    fid = np.nonzero(SN.valid_faces(v, SN._faces(f)))[0] if v.shape[0] else np.zeros(0, int)
    target = (lo + g.random((n, 3)) * ext).astype(F)
    if fid.size:
        tri = v[f[fid[g.integers(0, fid.size, 120)]]]                    # [120,3,3]
        c = g.integers(0, 3, 40)
        target[:40] = tri[np.arange(40), c]
        target[40:80] = (tri[40:80, 0] + tri[40:80, 1]) * F(0.5)
        w = g.dirichlet(np.ones(3), 40).astype(F)
        target[80:120] = (tri[80:120] * w[:, :, None]).sum(1)
    d = (target - o).astype(F)
    d[::3] *= F(0.37)                                                   # not unit, some short
    tmin = np.zeros(n, F)
    tmax = np.full(n, np.inf, F)
    tmin[5:80:16] = -np.inf                                            # the whole line,
    d[5:80:16] *= F(-1)                                                # the target behind
    tmax[7:80:16] = F(1.5)
    # axis-aligned rays, some through a vertex's coordinates
    ax_o = (lo - F(0.25) * ext + g.random((6, 3)) * ext * F(1.5)).astype(F)
    ax_d = np.zeros((6, 3), F)
    ax_d[np.arange(6), np.arange(6) % 3] = [1, 1, 1, -2, -0.5, -1]
    ax_o[np.arange(3), np.arange(3)] = (lo - ext)[np.arange(3)]
    ax_o[3 + np.arange(3), np.arange(3)] = (hi + ext)[np.arange(3)]
    if fid.size:
        ax_o[0, 1:] = v[f[fid[0], 0], 1:]
        ax_o[4, 0], ax_o[4, 2] = v[f[fid[-1], 1], 0], v[f[fid[-1], 1], 2]
    # in the plane z = 0.5 and across it
    pl_o = (lo + g.random((4, 3)) * ext).astype(F)
    pl_d = (g.random((4, 3)) - 0.5).astype(F)
    pl_o[:2, 2], pl_d[:2, 2] = 0.5, 0.0
    pl_o[2:, 2], pl_d[2:, 2] = lo[2] - F(1.0), [1.0, 0.75]
    bad_o = np.array([[np.nan, 0.5, 0.5], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], F)
    bad_d = np.array([[0, 0, 1], [0, 0, 0], [1, np.inf, 0]], F)
    O = np.concatenate([o, ax_o, pl_o, bad_o])
    Dr = np.concatenate([d, ax_d, pl_d, bad_d])
    tmin = np.concatenate([tmin, np.zeros(13, F)])
    tmax = np.concatenate([tmax, np.full(13, np.inf, F)])
    # t_max just short of, at and just beyond the hit of the first rays that hit
    _, t, _ = RN.raycast_mesh(v, f, O, Dr, tmin, tmax)
    k = np.nonzero(np.isfinite(t) & (t > 0))[0][:4]
    extra_t = np.concatenate([np.nextafter(t[k], F(0)), t[k], np.nextafter(t[k], F(np.inf))])
    O = np.concatenate([O, O[k], O[k], O[k]])
    Dr = np.concatenate([Dr, Dr[k], Dr[k], Dr[k]])
    tmin = np.concatenate([tmin, np.zeros(3 * k.size, F)])
    tmax = np.concatenate([tmax, extra_t.astype(F)])
    out = tuple(np.ascontiguousarray(a, F) for a in (O, Dr, tmin, tmax))
    for a in out:
        a.setflags(write=False)
    _RAYS[name] = out
    return out


def want(name):
    """the definition's answer, computed once and shared (read-only)"""
    if name not in _WANT:
        v, f, _, _ = all_cases()[name]
        out = RN.raycast_mesh(v, f, *rays_of(name))
        for a in out:
            a.setflags(write=False)
        _WANT[name] = out
    return _WANT[name]


def same(got, ref):
    return (got[0].dtype == np.int32 and got[1].dtype == F and got[2].dtype == F and
            got[2].shape == ref[2].shape and all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)))


@pytest.mark.parametrize("name", NAMES)
def test_traversal_model_equals_the_definition_at_three_cell_sizes_and_a_moved_origin(name):
    v, f, _, _ = all_cases()[name]
    O, Dr, tmin, tmax = rays_of(name)
    ref = want(name)
    occ = (ref[0] >= 0).astype(np.uint8)
    cells = cells_of(name)
    fin = v[np.isfinite(v).all(1)] if v.size else v
    moved = (fin.min(0) if fin.size else np.zeros(3, F)) - np.array([0.77, 0.31, 1.9], F)
    for cell, origin in [(c, None) for c in cells] + [(cells[2], moved)]:
        assert same(RN.raycast_grid(v, f, O, Dr, tmin, tmax, cell=cell, origin=origin), ref), (name, cell)
        got = RN.raycast_grid(v, f, O, Dr, tmin, tmax, cell=cell, origin=origin, any_hit=True)
        assert got.dtype == np.uint8 and got.tobytes() == occ.tobytes(), (name, cell)
    # scalar ranges and another ray order
    perm = np.random.default_rng(1).permutation(O.shape[0])
    ref0 = RN.raycast_mesh(v, f, O, Dr, 0.0, 2.0)
    got = RN.raycast_grid(v, f, O[perm], Dr[perm], 0.0, 2.0, cell=cells[1])
    assert all(a.tobytes() == b[perm].tobytes() for a, b in zip(got, ref0)), name


def test_the_rays_hold_what_they_are_for():
    for name in NAMES:
        O, Dr, tmin, tmax = rays_of(name)
        face, t, bary = want(name)
        n_extra = O.shape[0] - 161
        assert 0 <= n_extra <= 12 and (face[158:161] == -1).all(), name
        miss = face < 0
        assert np.isinf(t[miss]).all() and (bary[miss] == 0).all() and np.isfinite(t[~miss]).all()
        assert (t[~miss] >= tmin[~miss]).all() and (t[~miss] <= tmax[~miss]).all()
        if name in ("f0", "v0"):
            assert miss.all()
            continue
        assert n_extra == 12, name
        # short of the hit: another face or none; at the hit and beyond it: the hit itself
        k = np.nonzero(np.isfinite(t[:161]) & (t[:161] > 0))[0][:4]
        assert (t[161:165] < t[k]).all() or (face[161:165] != face[k]).any()
        assert not (t[161:165] == t[k]).any()
        assert (face[165:169] == face[k]).all() and (t[165:169] == t[k]).all()
        assert (face[169:173] == face[k]).all() and (t[169:173] == t[k]).all()
        if name != "flat":
            assert (~miss[:120]).mean() > 0.5, name
        assert (t[5:80:16] < 0).any(), name
    # rays in the plane of ``flat`` hit nothing; rays across it may
    face = want("flat")[0]
    assert (face[154:156] == -1).all()
    # corners, edges and interiors are all met: weights that are 0 and weights that are not
    bary = want("random")[2][want("random")[0] >= 0]
    assert (np.abs(bary) < 1e-6).any() and (bary.min(1) > 1e-3).any()


def test_the_walk_prunes():
    for name, share in (("room", 8), ("random", 8)):
        v, f, _, _ = all_cases()[name]
        st = {}
        got = RN.raycast_grid(v, f, *rays_of(name), cell=cells_of(name)[2], stats=st)
        assert same(got, want(name))
        n = rays_of(name)[0].shape[0]
        assert st["cells"] > 500 and st["cells_visited"] * share < n * st["cells"], (name, st)


# ---- watertightness ----------------------------------------------------------
def pinhole_rays(pose, K, H, W):
    """ops.get_rays' convention in float64: pixel (u, v) looks through
    ((u + 0.5 - cx) / fx, (v + 0.5 - cy) / fy, 1), normalised, rotated by the pose"""
    fx, fy, cx, cy = K
    u, vv = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    d = np.stack([(u - cx) / fx, (vv - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
    nrm = np.linalg.norm(d, axis=1, keepdims=True)
    d = (d / nrm) @ pose[:3, :3].T
    return np.broadcast_to(pose[:3, 3], d.shape).copy(), d, nrm[:, 0]


def room_views(n, H, W):
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import _slerp_loop_poses
    poses = _slerp_loop_poses(16).numpy().astype(np.float64)[:: 16 // n][:n]
    return poses, (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)


def test_watertight_on_shared_edges_and_vertices_and_inside_the_room():
    v, f, _, _ = all_cases()["shared"]
    tri = v[f[:30]]
    # points of the lattice surface that lie on no boundary edge: inner vertices and
    # the midpoints of the diagonals
    idx = np.arange(42).reshape(7, 6)[1:-1, 1:-1].reshape(-1)
    pts = np.concatenate([v[idx], (tri[:, 0] + tri[:, 2]) * F(0.5)]).astype(F)
    g = np.random.default_rng(3)
    for o in (np.array([0.4, 0.3, 2.0], F), np.array([0.1, 0.6, -1.5], F)):
        d = (pts - o).astype(F)
        face, t, bary = RN.raycast_mesh(v, f, np.broadcast_to(o, d.shape), d)
        assert (face >= 0).all() and (np.abs(t - 1) < 1e-5).all()
    # straight down through vertices and edge midpoints: sheared coordinates are exact
    # zeros there, the tie of the edge functions itself
    o = pts + np.array([0, 0, 1], F)
    d = np.broadcast_to(np.array([0, 0, -1], F), o.shape)
    face, t, bary = RN.raycast_mesh(v, f, o, d)
    assert (face >= 0).all() and (bary == 0).any(1).all()
    got = RN.raycast_grid(v, f, o, d, cell=cells_of("shared")[2])
    assert same(got, (face, t, bary))
    # a camera inside the room: no ray of a 24 x 32 view misses
    m = room()["coarse"]
    poses, K = room_views(1, 24, 32)
    ro, rd, _ = pinhole_rays(poses[0], K, 24, 32)
    face, t, _ = RN.raycast_grid(m["verts"], m["faces"], ro.astype(F), rd.astype(F))
    assert (face >= 0).all() and (t > 0).all()


# ---- an independent float64 cast -----------------------------------------------
def moller_trumbore(v, f, O, Dr):
    """float64, brute force -> (face, t, bary [N,3]); -1 where nothing is hit at t > 0"""
    V, Fc = np.asarray(v, np.float64), np.asarray(f)
    ok = SN.valid_faces(np.asarray(v, F), SN._faces(f))
    A, B, C = (V[Fc[ok, c]] for c in range(3))
    e1, e2 = B - A, C - A
    O, Dr = np.asarray(O, np.float64), np.asarray(Dr, np.float64)
    face = np.full(O.shape[0], -1, np.int64)
    t = np.full(O.shape[0], np.inf)
    bary = np.zeros((O.shape[0], 3))
    fid = np.nonzero(ok)[0]
    with np.errstate(all="ignore"):
        for i in range(O.shape[0]):
            p = np.cross(Dr[i], e2)
            det = (e1 * p).sum(1)
            s = O[i] - A
            u = (s * p).sum(1) / det
            q = np.cross(s, e1)
            w = (q * Dr[i]).sum(1) / det
            tt = (e2 * q).sum(1) / det
            hit = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (tt > 0)
            if hit.any():
                j = np.argmin(np.where(hit, tt, np.inf))
                face[i], t[i], bary[i] = fid[j], tt[j], (1 - u[j] - w[j], u[j], w[j])
    return face, t, bary


def t_bound(v, f, face, O, Dr, t):
    """The first-order bound on |t - t_exact| of a hit of ``face`` (derivation:
    docs/DESIGN_NOTEBOOK.md, section RC).  With u = 2^-24, m the largest
    |corner - o| component, n the face's unit normal and k the ray's major axis:
    each sheared corner is off by at most 6 u m in X and in Y (five float32
    roundings on operands no larger than 2 m); a plane n . (P - o) = c has
    t = (c - n_x X - n_y Y) / (n . d) in sheared coordinates, so those errors move
    t by at most 6 u m (|n_x| + |n_y|) / |n . d|; the rounded depths p_z move it by
    u m / |d_k|; the float64 sums add nothing at this order and the conversion to
    float32 adds u |t|.  A second u |t| covers the reference's own rounding."""
    V = np.asarray(v, np.float64)
    tri = V[np.asarray(f)[face]]                                         # [N,3,3]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    O, Dr = np.asarray(O, np.float64), np.asarray(Dr, np.float64)
    kz = np.argmax(np.abs(Dr), axis=1)
    rows = np.arange(O.shape[0])
    m = np.abs(tri - O[:, None, :]).max((1, 2))
    lateral = np.abs(n).sum(1) - np.abs(n[rows, kz])
    nd = np.abs((n * Dr).sum(1))
    return U * (m * (6.0 * lateral / nd + 1.0 / np.abs(Dr[rows, kz])) + 2.0 * np.abs(t))


def test_against_an_independent_float64_cast():
    """Measured here: every kept ray names the float64 cast's face; 40, 40, 40 and 38
    of the 40 rays per case are kept by the 1e-3 rule; the largest |t - t64| /
    ``t_bound`` is 0.11 (random), 0.14 (shifted), 0.12 (spanning), 0.41 (room)."""
    worst = {}
    for name in ("random", "shifted", "spanning", "room"):
        v, f, _, _ = all_cases()[name]
        O, Dr, _, _ = rays_of(name)
        O, Dr = O[INTERIOR], Dr[INTERIOR]
        face, t, bary = tuple(a[INTERIOR] for a in want(name))
        f64, t64, b64 = moller_trumbore(v, f, O, Dr)
        keep = (f64 >= 0) & (b64.min(1) >= 1e-3)
        assert keep.sum() >= 30, (name, keep.sum())
        assert (face[keep] == f64[keep]).all(), name
        err = np.abs(t[keep].astype(np.float64) - t64[keep])
        bound = t_bound(v, f, f64[keep], O[keep], Dr[keep], t64[keep])
        worst[name] = float((err / bound).max())
        assert (err <= bound).all(), (name, worst[name])
        assert np.abs(bary[keep] - b64[keep]).max() < 1e-3, name
    print("|t - t64| / bound:", worst)


def test_analytic_room():
    """The 466-face mesh under pinhole rays of 3 views at 24 x 32 against
    SyntheticRoom.cast on the same rays in float64.  The bound asserted on
    |t - t_analytic| is ``t_bound`` (first order in 2^-24, see there); measured
    here: 1 of 2304 rays left out by the 1e-4 rule, no class differing, the
    largest |t - t_analytic| / bound 0.56, |t - t_analytic| <= 1.37 2^-24 (|o|_inf + t)."""
    import torch
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    m = room()["coarse"]
    assert m["faces"].shape[0] == 466
    poses, K = room_views(3, 24, 32)
    ro, rd = (np.concatenate(x).astype(F) for x in
              list(zip(*[pinhole_rays(p, K, 24, 32)[:2] for p in poses])))
    face, t, bary = RN.raycast_grid(m["verts"], m["faces"], ro, rd)
    assert same((face, t, bary), RN.raycast_mesh(m["verts"], m["faces"], ro, rd))
    assert (face >= 0).all()
    ta, _, la = SyntheticRoom(0).cast(torch.from_numpy(ro).double(), torch.from_numpy(rd).double())
    ta, la = ta.numpy(), la.numpy()
    keep = bary.min(1) >= 1e-4
    left_out = int((~keep).sum())
    assert left_out <= 0.01 * keep.size, left_out
    assert (m["face_classes"][face[keep]] == la[keep]).all()
    err = np.abs(t[keep].astype(np.float64) - ta[keep])
    bound = t_bound(m["verts"], m["faces"], face[keep], ro[keep], rd[keep], ta[keep])
    rel = err / (U * (np.abs(ro[keep]).max(1) + ta[keep]))
    print("analytic room: left out", left_out, "err/bound", (err / bound).max(), "err/(u(|o|+t))", rel.max())
    assert (err <= bound).all(), float((err / bound).max())


# ---- hand cases ---------------------------------------------------------------
def test_hand_cases_ties_inclusive_range_start_on_a_face_and_the_box_clause():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F)
    o = np.array([[0.25, 0.25, 1.0]], F)
    d = np.array([[0, 0, -2]], F)
    for fn in (RN.raycast_mesh, RN.raycast_grid):
        # a duplicated face: the smaller index wins, both ways round
        for ff in ([[1, 3, 2], [0, 1, 2], [0, 1, 2]], [[0, 1, 2], [1, 3, 2], [0, 1, 2]]):
            face, t, bary = fn(v, np.array(ff, np.int32), o, d)
            assert face.tolist() == [ff.index([0, 1, 2])] and t.tolist() == [0.5]
            assert bary.tolist() == [[0.5, 0.25, 0.25]]
        f = np.array([[0, 1, 2]], np.int32)
        # the range is inclusive at both ends
        for tmin, tmax, hit in ((0.5, 1.0, True), (0.0, 0.5, True), (0.5, 0.5, True),
                                (np.nextafter(F(0.5), F(1)), 1.0, False),
                                (0.0, np.nextafter(F(0.5), F(0)), False), (np.nan, 1.0, False)):
            face, t, _ = fn(v, f, o, d, tmin, tmax)
            assert face.tolist() == [0 if hit else -1] and t.tolist() == [0.5 if hit else np.inf]
        # no culling: from below; a ray that starts on the face hits it at t = 0
        face, t, _ = fn(v, f, np.array([[0.25, 0.25, -1.0]], F), np.array([[0, 0, 1]], F))
        assert face.tolist() == [0] and t.tolist() == [1.0]
        face, t, _ = fn(v, f, np.array([[0.25, 0.25, 0.0]], F), np.array([[0.1, 0.2, 1]], F))
        assert face.tolist() == [0] and t.tolist() == [0.0]
        face, t, _ = fn(v, f, np.array([[0.25, 0.25, 0.0]], F), np.array([[0.1, 0.2, 1]], F), 1e-6)
        assert face.tolist() == [-1]
        # behind the origin only with a negative t_min
        face, t, _ = fn(v, f, o, -d)
        assert face.tolist() == [-1]
        face, t, _ = fn(v, f, o, -d, -np.inf)
        assert face.tolist() == [0] and t.tolist() == [-0.5]
        assert RN.mesh_occluded(v, f, o, d).tolist() == [1]
        assert RN.raycast_grid(v, f, o, -d, any_hit=True).tolist() == [0]
    # The box clause.  What the inside test promises is exact for the sheared corners,
    # and those carry the rounding of Sx * pz: about 4 * 2^-24 * |Sx| * (the face's reach along
    # the major axis).  A face in the plane x = 0 that reaches 1000 units along z, seen at
    # a slant from a point close to that plane, is "inside" with t = 0.4259 where the
    # ray's x is -6.3e-6: eleven times S = 2^-20 (|o_x| + |t d_x| + 0) outside the face's
    # own (flat) box in x.  The clause rejects it, and no traversal has to find it.  An
    # edge-on face's t is a convex sum of its corners' depths whatever the weights are,
    # so its point leaves the box by the same rounding and by nothing else.
    v = np.array([[0, -1, -1000], [0, 1, -1000], [0, 0, 1000]], F)
    f = np.array([[0, 1, 2]], np.int32)
    o = np.array([[-0.28473424911499023, -0.031345825642347336, -0.1309327632188797]], F)
    d = np.array([[0.6685235500335693, 0.09748899936676025, 1.0]], F)
    o3, d3 = tuple(o[:, a] for a in range(3)), tuple(d[:, a] for a in range(3))
    tri = tuple(tuple(v[c, a][None] for a in range(3)) for c in range(3))
    hit, t, Uu, Vv, W, det = RN.intersect(o3, d3, RN.major_axis(d3), *tri, F(0), F(np.inf))
    inside = ((Uu >= 0) & (Vv >= 0) & (W >= 0)) | ((Uu <= 0) & (Vv <= 0) & (W <= 0))
    px = o[0, 0] + t[0] * d[0, 0]
    S = RN.K * ((abs(o[0, 0]) + abs(t[0] * d[0, 0])) + F(0))
    assert inside[0] and det[0] != 0 and 0 < t[0] < 1 and not hit[0]
    assert abs(px) > 8 * S and abs(px) < 1e-5
    for fn in (RN.raycast_mesh, RN.raycast_grid):
        assert fn(v, f, o, d)[0].tolist() == [-1]
        assert fn(v, f, o, d, any_hit=True).tolist() == [0] if fn is RN.raycast_grid else True
        # the same face is hit by a ray whose shear is exact
        face, t1, _ = fn(v, f, np.array([[-1.0, 0.25, 3.0]], F), np.array([[1, 0, 0]], F))
        assert face.tolist() == [0] and t1.tolist() == [1.0]
