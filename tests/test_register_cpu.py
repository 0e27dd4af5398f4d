"""CPU-only: the host half of the registration (utils/registration.py:
normal_equations, solve_step, compose) over the numpy restatement of the fused
ICP step (tests/register_numpy.py): the summation tree's definition, convergence
of point-to-plane ICP on the analytic room to the float32 floor, the monotone
(and slow) decrease of point-to-point, a target that leaves three directions
free, and the composition."""
import math

import numpy as np
import pytest

from tests import register_numpy as RG
from tests.sdf_numpy import face_unit_normals
from ucsa_neural_rendering_amd.utils.registration import (compose, normal_equations,
                                                          rotation_angle, solve_step)

F = np.float32
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
_ROOM = {}


def rigid(angle_deg, shift, axis=AXIS, seed=0):
    """a rotation by ``angle_deg`` about ``axis`` and a shift of length ``shift`` -> 4x4"""
    d = np.random.default_rng(seed).normal(size=3)
    d *= shift / np.linalg.norm(d)
    return compose(np.eye(4), np.concatenate([np.radians(angle_deg) * axis, np.zeros(3)])) + \
        np.pad(d[:, None], ((0, 1), (3, 0)))


def room_mesh():
    """the 466-face room and its unit normals (shared: do not write)"""
    if not _ROOM:
        from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
        m = SyntheticRoom(0).labelled_mesh(1.0)
        v, f = np.asarray(m["verts"], F), np.asarray(m["faces"], np.int32)
        _ROOM["mesh"] = (v, f, face_unit_normals(v, f))
        for a in _ROOM["mesh"]:
            a.setflags(write=False)
    return _ROOM["mesh"]


def surface_points(v, f, n, seed):
    """``n`` area-uniform points on the mesh -> float32 [n,3]"""
    g = np.random.default_rng(seed)
    tri = v[f].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    pick = g.choice(f.shape[0], n, p=area / area.sum())
    a, b = g.random(n), g.random(n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    t = tri[pick]
    return (t[:, 0] + a[:, None] * (t[:, 1] - t[:, 0]) + b[:, None] * (t[:, 2] - t[:, 0])).astype(F)


def moved_source(n, angle_deg, shift, seed=5):
    """``n`` surface points of the room moved by the inverse of a known transform
    -> (points float32, the transform that brings them back)"""
    v, f, _ = room_mesh()
    T = rigid(angle_deg, shift)
    p = surface_points(v, f, n, seed).astype(np.float64)
    src = (p - T[:3, 3]) @ T[:3, :3]                       # R^T (p - t)
    return src.astype(F), T


def pose_error(T, want):
    D = T @ np.linalg.inv(want)
    return rotation_angle(D[:3, :3]), float(np.linalg.norm(T[:3, 3] - want[:3, 3]))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_tree_in_one_piece_equals_the_tree_group_by_group(n):
    g = np.random.default_rng(n)
    x = g.normal(size=(n, 3)) * 10.0 ** g.integers(-8, 8, size=(n, 3))
    whole = RG.tree_sum(x)
    rows = x
    while True:                       # the definition, one group of 256 at a time
        groups = max(1, -(-rows.shape[0] // 256))
        out = np.zeros((groups, 3))
        for k in range(groups):
            grp = np.zeros((256, 3))
            part = rows[256 * k:256 * k + 256]
            grp[:part.shape[0]] = part
            while grp.shape[0] > 1:
                grp = grp[0::2] + grp[1::2]
            out[k] = grp[0]
        rows = out
        if groups == 1:
            break
    assert bits(whole).tolist() == bits(rows[0]).tolist()
    if n == 0:
        assert bits(whole).tolist() == [0, 0, 0]


def test_a_lone_negative_zero_sums_to_positive_zero():
    x = np.full((1, 29), -0.0)
    assert np.signbit(x).all()
    assert bits(RG.tree_sum(x)).tolist() == [0] * 29
    # 256 of them fill a group: no padding meets them and the sign survives
    assert np.signbit(RG.tree_sum(np.full((256, 2), -0.0))).all()


# ---------------------------------------------------------------------------
# convergence
# ---------------------------------------------------------------------------
CASES = [(2000, 3.0, 0.05), (2000, 8.0, 0.2), (256, 3.0, 0.05), (256, 8.0, 0.2)]
_RUNS = {}


def run(n, angle, shift, mode, iterations=10):
    key = (n, angle, shift, mode)
    if key not in _RUNS:
        v, f, un = room_mesh()
        src, want = moved_source(n, angle, shift)
        T, hist = RG.register_points(src, v, f, un, max_dist=0.5, iterations=iterations, mode=mode)
        _RUNS[key] = (T, hist, want)
    return _RUNS[key]


@pytest.mark.parametrize("n,angle,shift", CASES)
def test_point_to_plane_reaches_the_float32_floor_in_ten_iterations(n, angle, shift):
    T, hist, want = run(n, angle, shift, 0)
    rot, trans = pose_error(T, want)
    _, _, sse, count = normal_equations(hist[-1])
    print(f"n={n} {angle} deg {shift}: rot {rot:.3e} rad, trans {trans:.3e}, "
          f"rmse {math.sqrt(sse / count):.3e}, matched {int(count)}")
    assert count == n
    assert rot <= 1e-5 and trans <= 1e-5


@pytest.mark.parametrize("n,angle,shift", CASES)
def test_point_to_point_rmse_falls_monotonically(n, angle, shift):
    _, hist, _ = run(n, angle, shift, 1)
    rmse = []
    for s in hist:
        _, _, sse, count = normal_equations(s)
        assert count % 3 == 0 and 0 < count <= 3 * n      # three rows per matched point
        rmse.append(math.sqrt(3.0 * sse / count))
    print(f"n={n} {angle} deg {shift}: rmse " + " ".join(f"{r:.4f}" for r in rmse))
    assert all(b < a for a, b in zip(rmse, rmse[1:]))


def test_a_single_rectangle_leaves_three_directions_free():
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], F)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    un = face_unit_normals(v, f)
    g = np.random.default_rng(9)
    src = np.concatenate([g.uniform(-0.8, 0.8, (300, 2)), np.zeros((300, 1))], 1)
    T0 = rigid(2.0, 0.03, seed=4)
    src = ((src - T0[:3, 3]) @ T0[:3, :3]).astype(F)
    sums = RG.icp_sums(v, f, un, src, np.eye(4), 0.5, 0)[0]
    xi, rank = solve_step(sums)
    assert rank == 3
    free = np.abs(xi[[2, 3, 4]])                   # rotation about z, shifts along x and y
    assert free.max() <= 1e-12 * np.abs(xi).max()
    assert np.abs(xi[[0, 1, 5]]).min() > 1e-4
    T, hist = RG.register_points(src, v, f, un, max_dist=0.5, iterations=5)
    assert np.isfinite(T).all() and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
    _, _, sse, count = normal_equations(hist[-1])
    assert count == 300 and math.sqrt(sse / count) < 1e-6


# ---------------------------------------------------------------------------
# compose
# ---------------------------------------------------------------------------
def test_compose_with_zero_is_the_identity_to_the_bit():
    T = rigid(37.0, 1.5, seed=2)
    T[0, 3] = -0.0
    assert bits(compose(T, np.zeros(6))).tolist() == bits(T).tolist()
    assert bits(compose(T[:3], np.zeros(6))).tolist() == bits(T).tolist()


def test_rotation_stays_orthonormal_over_a_hundred_compositions():
    g = np.random.default_rng(1)
    T = np.eye(4)
    for _ in range(100):
        T = compose(T, g.normal(size=6) * 0.3)
    R = T[:3, :3]
    # a product of two rotations adds at most about 3 eps to R^T R - I: 300 eps = 7e-14
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-13
    assert T[3].tolist() == [0, 0, 0, 1]
    # exp is the exponential: two steps along one twist add up
    xi = g.normal(size=6) * 0.2
    assert np.abs(compose(compose(np.eye(4), xi), xi) - compose(np.eye(4), 2 * xi)).max() <= 1e-14
