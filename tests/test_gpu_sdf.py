"""GPU: signed distance to a mesh (csrc/mesh_sdf.hip: ucsa_face_unit_normals,
ucsa_normal_runs, ucsa_mesh_sign, ucsa_mesh_tsdf; ops.mesh_pseudonormals,
ops.signed_distance, ops.mesh_tsdf) against tests/sdf_numpy.py, byte for byte,
at three cell sizes, with sorted and unsorted queries; guard words, sentinels in
the voxels outside the band, unchanged inputs, argument codes; an analytic
sphere through ops.marching_cubes and ops.mesh_tsdf end to end; the signed
entries of utils/mesh_eval.mesh_distance and of scripts/score_mesh_3d.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import sdf_numpy as S
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded

pytestmark = pytest.mark.gpu
F = np.float32
MESHES = ("tetrahedron", "cube", "l_prism", "open_patch", "broken_mesh", "fan")
MAX_DIST = 1.5
CELLS = (None, 0.3, 2.5)


def mesh_of(name):
    made = getattr(S, name)()
    return np.ascontiguousarray(made[0], F), np.ascontiguousarray(made[1], np.int32)


def queries_of(V, Fc):
    """3 000: the finite vertices, edge midpoints and face centroids of the valid
    faces, random points of which many lie beyond MAX_DIST, and a NaN query"""
    rng = np.random.default_rng(5)
    ok = S.valid_faces(V, Fc)
    P = V[Fc[ok]]                                                     # [F',3,3]
    mid = ((P + P[:, [1, 2, 0]]) * F(0.5)).reshape(-1, 3)
    cen = ((P[:, 0] + P[:, 1]) + P[:, 2]) / F(3)
    special = np.concatenate([V[np.isfinite(V).all(1)], mid, cen]).astype(F)
    q = rng.uniform(-3, 3, (3000, 3)).astype(F)
    q[:special.shape[0]] = special
    q[-1] = (0.5, np.nan, 0.5)
    return q, special.shape[0]


def gpu_normals(V, Fc):
    N = _ops().mesh_pseudonormals(_cu(V).view(-1, 3), _cu(Fc).view(-1, 3))
    for k, shape in (("unit_normal", (Fc.shape[0], 3)), ("corner_angle", (Fc.shape[0], 3)),
                     ("vertex_normal", (V.shape[0], 3)), ("edge_normal", (Fc.shape[0], 3, 3))):
        assert N[k].dtype == torch.float32 and tuple(N[k].shape) == shape and N[k].is_contiguous()
    return N


_refs = {}


def reference(name):
    """(V, Fc, queries, n_special, the op's normals, the restatement fed the op's
    corner angles, its signed distance), computed once"""
    if name not in _refs:
        V, Fc = mesh_of(name)
        q, n_special = queries_of(V, Fc)
        N = gpu_normals(V, Fc)
        ref_n = S.pseudonormals(V, Fc, N["corner_angle"].cpu().numpy())
        _refs[name] = (V, Fc, q, n_special, N, ref_n, S.signed_distance(V, Fc, ref_n, q, MAX_DIST))
    return _refs[name]


def same_bytes(got, ref):
    return all(g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
               for g, r in zip(got, ref))


@pytest.mark.parametrize("name", MESHES)
def test_normals_equal_the_restatement_byte_for_byte(name):
    V, Fc, _, _, N, ref_n, _ = reference(name)
    for k in ("unit_normal", "vertex_normal", "edge_normal"):
        assert N[k].cpu().numpy().tobytes() == ref_n[k].tobytes(), (name, k)
    ok = S.valid_faces(V, Fc)
    ang = N["corner_angle"].cpu().numpy()
    assert (ang[~ok] == 0).all() and np.isfinite(ang).all()
    # the angles are torch's: an input of the contract, held to the formula only
    np.testing.assert_allclose(ang, S.corner_angles(V, Fc), rtol=0, atol=8 * 2.0 ** -23)


@pytest.mark.parametrize("name", MESHES)
def test_signed_distance_equals_the_restatement_at_three_cells_and_both_orders(name):
    ops = _ops()
    V, Fc, q, n_special, N, _, ref = reference(name)
    sdf_r, face_r, dist2_r, _, feat_r = ref
    Vg, Fg, Q = _cu(V).view(-1, 3), _cu(Fc).view(-1, 3), _cu(q).view(-1, 3)
    for cell in CELLS:
        grid = ops.triangle_grid(Vg, Fg, cell)
        near = ops.nearest_triangle(grid, Q, MAX_DIST)
        for sort_queries in (True, False):
            got = ops.signed_distance(grid, N, Vg, Fg, Q, MAX_DIST, sort_queries=sort_queries)
            assert got[0].dtype == torch.float32 and got[4].dtype == torch.int32
            assert same_bytes([t.cpu().numpy() for t in got], ref), (name, cell, sort_queries)
            # |sdf| is the search's distance, bit for bit
            assert torch.equal(got[0].abs().view(torch.int32), near[1].sqrt().view(torch.int32))
    miss = face_r < 0
    assert miss.sum() > 300 and np.isposinf(sdf_r[miss]).all() and (feat_r[miss] == -1).all()
    assert miss[-1]                                                   # the NaN query
    hit = ~miss
    assert (feat_r[hit] >= 0).all() and (feat_r[hit] <= 6).all()
    assert np.abs(sdf_r[hit]).tobytes() == np.sqrt(dist2_r[hit]).tobytes()
    # on the surface: +0.  The vertices are exact in every mesh, the edge
    # midpoints and face centroids in the cube (dyadic coordinates, axis planes)
    nv = int(np.isfinite(V).all(1).sum())
    used = np.unique(Fc[S.valid_faces(V, Fc)])
    at_vertex = np.isin(np.nonzero(np.isfinite(V).all(1))[0], used)
    zero = sdf_r[:nv][at_vertex]
    assert (zero == 0).all() and not np.signbit(zero).any()
    if name == "cube":
        assert (sdf_r[:nv + 36] == 0).all() and not np.signbit(sdf_r[:nv + 36]).any()
        assert np.abs(sdf_r[nv + 36:n_special]).max() < 1e-6          # centroids: a division by 3
    if name in ("tetrahedron", "cube", "l_prism"):
        assert (np.bincount(feat_r[hit], minlength=7) > 0).all()
        inside = getattr(S, name)()[2](q[hit].astype(np.float64))
        scored = np.abs(sdf_r[hit]) > 1e-4
        assert ((sdf_r[hit] < 0) == inside)[scored].all()


def raw_normal_runs(l, items, first, n_runs, n_items, weight, unit, nf, out):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    return l.ucsa_normal_runs(p(items), p(first), n_runs, n_items, p(weight), p(unit), nf, p(out),
                              None)


def test_entry_points_write_their_rows_only_and_leave_inputs_alone():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    V, Fc, q, _, N, ref_n, ref = reference("broken_mesh")
    nv, nf, nq = V.shape[0], Fc.shape[0], q.shape[0]
    Vg, Fg, Q = _cu(V).view(-1, 3), _cu(Fc).view(-1, 3), _cu(q).view(-1, 3)
    unit, check_u = guarded((nf, 3), torch.float32, -5.0)
    assert l.ucsa_face_unit_normals(p(Vg), nv, p(Fg), nf, p(unit), None) == 0
    torch.cuda.synchronize()
    check_u()
    assert unit.cpu().numpy().tobytes() == ref_n["unit_normal"].tobytes()
    # runs: malformed offsets and items, as tests/test_sdf_cpu.py feeds the restatement
    u2 = _cu(np.array([[1, 0, 0], [0, 1, 0]], F))
    w = _cu(np.arange(6).astype(F))
    items = _cu(np.array([0, 3, 7, -1, 4, 1], np.int32))
    first = _cu(np.array([-5, 2, 2, 99], np.int32))
    out, check_o = guarded((3, 3), torch.float32, -5.0)
    for weight in (w, None):
        assert raw_normal_runs(l, items, first, 3, 6, weight, u2, 2, out) == 0
        torch.cuda.synchronize()
        check_o()
        want = S.normal_runs(items.cpu().numpy(), first.cpu().numpy(), 3,
                             None if weight is None else w.cpu().numpy(), u2.cpu().numpy())
        assert out.cpu().numpy().tobytes() == want.tobytes()
    # the vertex runs of the mesh through the raw entry point
    it, fi = S.vertex_runs(V, Fc)
    ang = N["corner_angle"].reshape(-1).contiguous()
    vn, check_v = guarded((nv, 3), torch.float32, -5.0)
    assert raw_normal_runs(l, _cu(it), _cu(fi), nv, it.size, ang, unit, nf, vn) == 0
    torch.cuda.synchronize()
    check_v()
    assert vn.cpu().numpy().tobytes() == ref_n["vertex_normal"].tobytes()
    # the sign: faces out of range, invalid faces and the search's own
    face = ref[1].copy()
    face[:6] = [-1, nf, 2 ** 31 - 1, 6, 7, -2 ** 31]                   # 6, 7: invalid faces
    want_s, want_f = S.mesh_sign(V, Fc, ref_n, q, face)
    assert np.isposinf(want_s[:6]).all() and (want_f[:6] == -1).all()
    sdf, check_s = guarded((nq,), torch.float32, -5.0)
    feat, check_f = guarded((nq,), torch.int32, -5)
    Fa = _cu(face)
    assert l.ucsa_mesh_sign(p(Vg), nv, p(Fg), nf, p(N["unit_normal"]), p(N["vertex_normal"]),
                            p(N["edge_normal"]), p(Q), nq, p(Fa), p(sdf), p(feat), None) == 0
    torch.cuda.synchronize()
    check_s()
    check_f()
    assert sdf.cpu().numpy().tobytes() == want_s.tobytes()
    assert feat.cpu().numpy().tobytes() == want_f.tobytes()
    assert (Vg.cpu().numpy().tobytes() == V.tobytes() and Fg.cpu().numpy().tobytes() == Fc.tobytes()
            and Q.cpu().numpy().tobytes() == q.tobytes() and Fa.cpu().numpy().tobytes() == face.tobytes())
    for k in ("unit_normal", "vertex_normal", "edge_normal"):
        assert N[k].cpu().numpy().tobytes() == ref_n[k].tobytes()


# ---- the volume ---------------------------------------------------------------
DIMS, ORIGIN, SPACING = (24, 20, 18), (-1.45, 1.2, -1.05), (0.12, -0.12, 0.12)
TRUNC = 0.36                                                          # three voxels


def guarded_volume(tsdf_fill=7.0, weight_fill=-3.0):
    tsdf, check_t = guarded(DIMS, torch.float32, tsdf_fill)
    weight, check_w = guarded(DIMS, torch.float32, weight_fill)
    vol = {"tsdf": tsdf, "weight": weight, "rgb": None, "origin": ORIGIN, "spacing": SPACING}
    return vol, lambda: (check_t(), check_w())


@pytest.mark.parametrize("name", ("l_prism", "broken_mesh"))
def test_mesh_tsdf_equals_the_brute_force_and_the_materialised_lattice(name):
    ops = _ops()
    V, Fc, _, _, N, ref_n, _ = reference(name)
    Vg, Fg = _cu(V).view(-1, 3), _cu(Fc).view(-1, 3)
    t0, w0 = np.full(DIMS, 7, F), np.full(DIMS, -3, F)
    want_t, want_w = S.mesh_tsdf(t0, w0, ORIGIN, SPACING, V, Fc, ref_n, TRUNC, 2.5)
    band = want_w == F(2.5)
    assert 1000 < band.sum() < band.size - 1000                       # both kinds of voxel
    assert (want_t[~band] == 7).all() and (want_w[~band] == -3).all()
    assert (want_t[band] < 0).any() and (want_t[band] > 0).any() and (np.abs(want_t[band]) <= 1).all()
    pts = S.lattice_points(DIMS, ORIGIN, SPACING)
    for cell in CELLS:
        grid = ops.triangle_grid(Vg, Fg, cell)
        keep = {k: grid[k].clone() for k in ("records", "offsets")}
        vol, check = guarded_volume()
        assert ops.mesh_tsdf(vol, Vg, Fg, TRUNC, weight=2.5, grid=grid, normals=N) is vol
        torch.cuda.synchronize()
        check()
        assert vol["tsdf"].cpu().numpy().tobytes() == want_t.tobytes(), (name, cell)
        assert vol["weight"].cpu().numpy().tobytes() == want_w.tobytes(), (name, cell)
        for k, t in keep.items():
            assert torch.equal(grid[k].view(torch.int32), t.view(torch.int32)), k
        # the same search from a queries array
        sdf, face, _, _, _ = ops.signed_distance(grid, N, Vg, Fg, _cu(pts).view(-1, 3), TRUNC)
        hit = (face >= 0).view(DIMS)
        assert torch.equal(hit.cpu(), torch.from_numpy(band))
        # (the division in numpy: torch divides by a scalar through its reciprocal)
        t = np.clip(sdf.cpu().numpy().reshape(DIMS)[band] / F(TRUNC), F(-1), F(1))
        assert t.dtype == F and t.tobytes() == vol["tsdf"].cpu().numpy()[band].tobytes()
    assert Vg.cpu().numpy().tobytes() == V.tobytes() and Fg.cpu().numpy().tobytes() == Fc.tobytes()
    for k in ("unit_normal", "vertex_normal", "edge_normal"):
        assert N[k].cpu().numpy().tobytes() == ref_n[k].tobytes()
    # grid and normals built inside, the default weight
    vol, check = guarded_volume()
    ops.mesh_tsdf(vol, Vg, Fg, TRUNC)
    torch.cuda.synchronize()
    check()
    assert vol["tsdf"].cpu().numpy().tobytes() == want_t.tobytes()
    assert (vol["weight"].cpu().numpy()[band] == 1).all()


def test_argument_codes_come_before_any_launch():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f3, u3 = (lambda *x: (C.c_float * 3)(*x)), (lambda *x: (C.c_uint32 * 3)(*x))
    nan, inf = float("nan"), float("inf")
    V, Fc, q, _, N, _, ref = reference("l_prism")
    nv, nf, nq = V.shape[0], Fc.shape[0], 65
    Vg, Fg, Q = _cu(V).view(-1, 3), _cu(Fc).view(-1, 3), _cu(q[:nq]).view(-1, 3)
    grid = ops.triangle_grid(Vg, Fg)
    vol, check_vol = guarded_volume(99.0, 99.0)
    rec_off = torch.empty(grid["records"].numel() + 1, dtype=torch.float32, device="cuda")[1:]

    def tsdf_call(**over):
        a = dict(rec=grid["records"], off=grid["offsets"], n=grid["n_pairs"],
                 origin=f3(*grid["origin"]), cell=grid["cell"], dims=u3(*grid["dims"]), v=Vg, nv=nv,
                 f=Fg, nf=nf, un=N["unit_normal"], vn=N["vertex_normal"], en=N["edge_normal"],
                 tsdf=vol["tsdf"], weight=vol["weight"], nx=DIMS[0], ny=DIMS[1], nz=DIMS[2],
                 vo=f3(*ORIGIN), vs=f3(*SPACING), trunc=TRUNC, wv=1.0)
        a.update(over)
        return l.ucsa_mesh_tsdf(p(a["rec"]), p(a["off"]), a["n"], a["origin"], a["cell"], a["dims"],
                                p(a["v"]), a["nv"], p(a["f"]), a["nf"], p(a["un"]), p(a["vn"]),
                                p(a["en"]), p(a["tsdf"]), p(a["weight"]), a["nx"], a["ny"], a["nz"],
                                a["vo"], a["vs"], a["trunc"], a["wv"], None)
    for over, arg in ((dict(rec=None), 0), (dict(rec=rec_off), 0), (dict(off=None), 1),
                      (dict(n=2 ** 31), 2), (dict(origin=None), 3), (dict(origin=f3(0, nan, 0)), 3),
                      (dict(cell=0.0), 4), (dict(cell=nan), 4), (dict(dims=None), 5),
                      (dict(dims=u3(4, 0, 4)), 5), (dict(dims=u3(257, 256, 256)), 5),
                      (dict(v=None), 6), (dict(nv=2 ** 31), 7), (dict(f=None), 8),
                      (dict(nf=2 ** 31), 9), (dict(un=None), 10), (dict(vn=None), 11),
                      (dict(en=None), 12), (dict(tsdf=None), 13), (dict(weight=None), 14),
                      (dict(nx=1), 15), (dict(nz=0), 15), (dict(nx=65536, ny=65536), 15),
                      (dict(nx=2048, ny=2048, nz=512), 15), (dict(vo=None), 18), (dict(vs=None), 19),
                      (dict(trunc=0.0), 20), (dict(trunc=-1.0), 20), (dict(trunc=nan), 20),
                      (dict(trunc=inf), 20), (dict(trunc=1e20), 20)):
        assert tsdf_call(**over) == -(1000 + arg), (over, arg)
    assert tsdf_call(rec=None, off=None, n=0) == 0                     # no pairs: nothing written
    sdf, check_s = guarded((nq,), torch.float32, 99.0)
    feat, check_f = guarded((nq,), torch.int32, 99)
    face = _cu(ref[1][:nq])

    def sign_call(**over):
        a = dict(v=Vg, nv=nv, f=Fg, nf=nf, un=N["unit_normal"], vn=N["vertex_normal"],
                 en=N["edge_normal"], q=Q, nq=nq, face=face, sdf=sdf, feat=feat)
        a.update(over)
        return l.ucsa_mesh_sign(p(a["v"]), a["nv"], p(a["f"]), a["nf"], p(a["un"]), p(a["vn"]),
                                p(a["en"]), p(a["q"]), a["nq"], p(a["face"]), p(a["sdf"]),
                                p(a["feat"]), None)
    for over, arg in ((dict(v=None), 0), (dict(nv=2 ** 31), 1), (dict(f=None), 2),
                      (dict(nf=2 ** 31), 3), (dict(un=None), 4), (dict(vn=None), 5),
                      (dict(en=None), 6), (dict(q=None), 7), (dict(nq=2 ** 31), 8),
                      (dict(face=None), 9), (dict(sdf=None), 10), (dict(feat=None), 11)):
        assert sign_call(**over) == -(1000 + arg), (over, arg)
    assert sign_call(q=None, nq=0, face=None, sdf=None, feat=None) == 0
    unit, check_u = guarded((nf, 3), torch.float32, 99.0)
    for args, arg in (((None, nv, p(Fg), nf, p(unit)), 0), ((p(Vg), 2 ** 31, p(Fg), nf, p(unit)), 1),
                      ((p(Vg), nv, None, nf, p(unit)), 2), ((p(Vg), nv, p(Fg), 2 ** 31, p(unit)), 3),
                      ((p(Vg), nv, p(Fg), nf, None), 4)):
        assert l.ucsa_face_unit_normals(*args, None) == -(1000 + arg), arg
    assert l.ucsa_face_unit_normals(None, 0, None, 0, None, None) == 0
    it, fi = S.vertex_runs(V, Fc)
    items, first = _cu(it), _cu(fi)
    out, check_o = guarded((nv, 3), torch.float32, 99.0)
    run = lambda **o: raw_normal_runs(l, **{**dict(items=items, first=first, n_runs=nv,
                                                   n_items=it.size, weight=None,
                                                   unit=N["unit_normal"], nf=nf, out=out), **o})
    for over, arg in ((dict(items=None), 0), (dict(first=None), 1), (dict(n_runs=2 ** 31), 2),
                      (dict(n_items=2 ** 31), 3), (dict(unit=None), 5),
                      (dict(nf=(2 ** 31 - 1) // 3 + 1), 6), (dict(out=None), 7)):
        assert run(**over) == -(1000 + arg), (over, arg)
    assert run(items=None, first=None, n_runs=0, out=None) == 0
    torch.cuda.synchronize()
    for c in (check_vol, check_s, check_f, check_u, check_o):
        c()
    for t in (vol["tsdf"], vol["weight"], sdf, feat, unit, out):
        assert (t == 99).all()                                        # nothing was launched
    other = ops.mesh_pseudonormals(*(_cu(a).view(-1, 3) for a in mesh_of("cube")))
    plain = ops.tsdf_volume(DIMS, ORIGIN, SPACING)
    for bad in (lambda: ops.mesh_pseudonormals(Vg.cpu(), Fg), lambda: ops.mesh_pseudonormals(Vg, Fg.long()),
                lambda: ops.mesh_pseudonormals(Vg, Fg[:, :2]),
                lambda: ops.signed_distance(grid, other, Vg, Fg, Q, 0.5),
                lambda: ops.signed_distance(grid, {"unit_normal": N["unit_normal"]}, Vg, Fg, Q, 0.5),
                lambda: ops.signed_distance(grid, N, Vg, Fg[:4], Q, 0.5),
                lambda: ops.signed_distance(grid, N, Vg, Fg, Q, 0.0),
                lambda: ops.mesh_tsdf(plain, Vg, Fg, 0.0), lambda: ops.mesh_tsdf(plain, Vg, Fg, inf),
                lambda: ops.mesh_tsdf(plain, Vg, Fg, 0.3, weight=nan),
                lambda: ops.mesh_tsdf(plain, Vg, Fg, 0.3, normals=other),
                lambda: ops.mesh_tsdf(plain, Vg, Fg[:4], 0.3, grid=grid),
                lambda: ops.mesh_tsdf(plain, Vg.cpu(), Fg.cpu(), 0.3)):
        with pytest.raises(UcsaError):
            bad()


# ---- an analytic sphere, end to end ---------------------------------------------
H, N_AX = 0.1, 21
# The centre is in general position on purpose.  With it on a lattice point the
# field equals iso at lattice points ((0.6, 0, 0), (0.4, 0.4, 0.2), ...), marching
# cubes emits coincident vertices and zero-area faces there, and the theorem
# behind the pseudonormal does not cover such a mesh (README, "Signed distance").
CENTRE = (0.013, -0.021, 0.037)


def sphere_field(R):
    ax = -1.0 + np.arange(N_AX) * H
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return np.sqrt((X - CENTRE[0]) ** 2 + (Y - CENTRE[1]) ** 2 + (Z - CENTRE[2]) ** 2) - R


def sphere_mesh(R):
    """ops.marching_cubes of -sdf at iso 0, as utils.tsdf_fusion.extract_mesh
    meshes a volume: matter is where the field is above iso"""
    out = _ops().marching_cubes(_cu((-sphere_field(R)).astype(F)), 0.0, (-1.0, -1.0, -1.0),
                                (H, H, H))
    return out[0].contiguous(), out[1].to(torch.int32).contiguous()


def test_sphere_through_marching_cubes_and_mesh_tsdf():
    """| |sdf| - |analytic| | <= h^2 / R in the band: the chord sag of a triangle
    of side up to sqrt(3) h on a sphere, 3 h^2 / 8 R, plus the error of placing a
    vertex by linear interpolation of a field whose second derivative along an
    edge is at most 1 / (R - h), h^2 / 8 (R - h).  The sign is unanimous: a
    marching-cubes mesh is counter-clockwise seen from the side where the field
    is below iso, so with field = -sdf the positive side is outside, and
    mesh_tsdf's sign is the analytic one (measured in the restatement on the
    CPU: largest distance error 0.0059 against the bound 0.0167, 0 wrong signs
    of 2 454)."""
    ops = _ops()
    R = 0.6
    an = sphere_field(R)
    verts, faces = sphere_mesh(R)
    assert 1000 < faces.shape[0] < 2000
    trunc = 3 * H
    vol = ops.tsdf_volume((N_AX,) * 3, (-1.0, -1.0, -1.0), H)
    ops.mesh_tsdf(vol, verts, faces, trunc)
    w = vol["weight"].cpu().numpy()
    sd = vol["tsdf"].cpu().numpy().astype(np.float64) * trunc
    band = w > 0
    assert set(np.unique(w)) == {0.0, 1.0} and (vol["tsdf"].cpu().numpy()[~band] == 1).all()
    assert band[np.abs(an) < trunc - H * H / R].all() and not band[np.abs(an) > trunc + H * H / R].any()
    inner = band & (np.abs(sd) < trunc)                               # not clamped
    err = np.abs(np.abs(sd[inner]) - np.abs(an[inner]))
    print("sphere: band", int(band.sum()), "largest error", err.max(), "bound", H * H / R)
    assert err.max() <= H * H / R
    far = band & (np.abs(an) > H / 2)
    agree = np.sign(sd[far]) == np.sign(an[far])
    print("sphere: voxels scored for the sign", int(far.sum()), "agreeing", int(agree.sum()))
    assert far.sum() > 2000 and (an[far] < 0).any() and (an[far] > 0).any()
    assert agree.all() or not agree.any()                             # one global orientation
    assert agree.all()                                                # and it is this one
    # the volume goes where a fused volume goes: re-meshed, it is the sphere again
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import extract_mesh, volume_from_mesh
    v2 = extract_mesh(vol)[0].cpu().numpy().astype(np.float64)
    r2 = np.linalg.norm(v2 - np.array(CENTRE), axis=1)
    assert v2.shape[0] > 300 and np.abs(r2 - R).max() <= 2 * H * H / R
    made = volume_from_mesh(verts, faces, H, trunc)
    o = np.asarray(made["origin"])
    lo = verts.min(0).values.cpu().numpy()
    assert made["spacing"] == (H,) * 3 or np.allclose(made["spacing"], H)
    assert np.allclose(o, lo - (np.float32(trunc) + np.float32(H)), atol=1e-6)
    mw = made["weight"].cpu().numpy()
    assert set(np.unique(mw)) == {0.0, 1.0} and (mw[0] == 0).all() and (mw[-1] == 0).all()
    assert (mw[:, 0] == 0).all() and (mw[:, -1] == 0).all() and (mw[:, :, 0] == 0).all() \
        and (mw[:, :, -1] == 0).all()                                 # the band fits in the pad
    mt = made["tsdf"].cpu().numpy()
    assert (mt[mw > 0] < 0).any() and (mt[mw > 0] > 0).any()


def test_mesh_distance_signed_tells_inside_from_outside(tmp_path, capsys):
    from scripts import score_mesh_3d
    from ucsa_neural_rendering_amd.utils.mesh_eval import mesh_distance, tsdf_bias
    from ucsa_neural_rendering_amd.utils.ply import write_ply
    ops = _ops()
    R, tol = 0.6, H * H / 0.6
    pv, pf = sphere_mesh(R)
    gv, gf = sphere_mesh(0.65)
    plain = mesh_distance(pv, gv, 0.1, 0.3, pred_faces=pf, gt_faces=gf)
    got = mesh_distance(pv, gv, 0.1, 0.3, pred_faces=pf, gt_faces=gf, signed=True)
    assert {k: got[k] for k in plain} == plain
    assert sorted(set(got) - set(plain)) == ["behind_share", "signed_mean", "signed_median"]
    print("signed:", {k: got[k] for k in ("signed_mean", "signed_median", "behind_share")})
    # the smaller sphere lies behind the larger one's outward faces
    assert abs(got["signed_mean"] + 0.05) <= tol and abs(got["signed_median"] + 0.05) <= tol
    assert got["behind_share"] == 1.0
    assert abs(abs(got["signed_mean"]) - got["accuracy"]) < 1e-6
    flipped = mesh_distance(pv, gv, 0.1, 0.3, gt_faces=gf[:, [0, 2, 1]].contiguous(), signed=True)
    assert abs(flipped["signed_mean"] - 0.05) <= tol and flipped["behind_share"] == 0.0
    outer = mesh_distance(gv, pv, 0.1, 0.3, gt_faces=pf, signed=True)
    assert abs(outer["signed_mean"] - 0.05) <= tol and outer["behind_share"] == 0.0
    with pytest.raises(ValueError):
        mesh_distance(pv, gv, 0.1, 0.3, signed=True)
    assert "signed_mean" not in mesh_distance(pv, gv, 0.1, 0.3)
    # a volume made from the smaller sphere against the larger mesh: the fused
    # surface lies behind the mesh by 0.05
    trunc = 3 * H
    vol = ops.mesh_tsdf(ops.tsdf_volume((N_AX,) * 3, (-1.0, -1.0, -1.0), H), pv, pf, trunc)
    bias = tsdf_bias(vol, gv, gf, trunc)
    inner = tsdf_bias(vol, pv, pf, trunc)
    assert inner["n"] > 2000 and inner["mean"] == 0 and inner["mean_abs"] == 0
    assert bias["n"] > 2000 and bias["mean"] > 0 and abs(bias["median"] - 0.05) <= 2 * tol
    assert bias["mean_abs"] >= abs(bias["mean"])
    # the script
    write_ply(str(tmp_path / "p.ply"), pv.cpu().numpy(), pf.cpu().numpy())
    write_ply(str(tmp_path / "g.ply"), gv.cpu().numpy(), gf.cpu().numpy())
    args = ["--pred", str(tmp_path / "p.ply"), "--gt", str(tmp_path / "g.ply"),
            "--max_dist", "0.3", "--threshold", "0.1"]
    capsys.readouterr()
    rec = score_mesh_3d.main(args + ["--signed"])
    out = capsys.readouterr().out.splitlines()
    geo = mesh_distance(pv, gv, 0.1, 0.3, gt_faces=gf, signed=True)
    assert out == ["geometry: " + json.dumps(geo)] and rec["geometry"] == geo
    assert geo["surface"] == (True, False) and geo["behind_share"] == 1.0
    rec = score_mesh_3d.main(args + ["--signed", "--surface"])
    assert capsys.readouterr().out.splitlines() == ["geometry: " + json.dumps(got)]
    rec = score_mesh_3d.main(args)                                     # the former line
    out = capsys.readouterr().out.splitlines()
    assert out == ["geometry: " + json.dumps(mesh_distance(pv, gv, 0.1, 0.3))]
    assert "signed" not in out[0] and "behind" not in out[0] and "surface" not in out[0]
    with pytest.raises(SystemExit):
        score_mesh_3d.main(args + ["--signed", "--sample_density", "100"])
