"""numpy restatement of the fused ICP step (csrc/mesh_register.hip:
ucsa_icp_sums; ops.register.icp_sums) and of the loop around it
(utils.registration.register_points).

The search is tests/surface_numpy.py's brute force over all faces, so a result
cannot depend on a cell grid.  The transform, the closest point, r and J are the
contract's float32 expressions as written, nothing fused; the 29 terms per point
are float64 products of converted floats, and the sum is the contract's tree:
rows padded with +0.0 to a multiple of 256, every 256 reduced by eight levels
of ``x[0::2] + x[1::2]``, repeated until one row is left."""
import numpy as np

from tests.nearest_numpy import F, _f32
from tests.surface_numpy import _faces, closest, nearest_triangle

SUMS = 29
PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]


def transform_points(points, transform):
    """q_k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k] in float32 -> [N,3]"""
    P = _f32(points)
    T = np.asarray(transform, np.float64)[:3].astype(F)
    with np.errstate(all="ignore"):
        q = [((T[k, 0] * P[:, 0] + T[k, 1] * P[:, 1]) + T[k, 2] * P[:, 2]) + T[k, 3]
             for k in range(3)]
    q = np.stack(q, 1)
    assert q.dtype == F
    return q


def tree_sum(terms):
    """float64 [N,C] -> [C]: the fixed tree of the contract"""
    x = np.ascontiguousarray(terms, np.float64)
    x = x.reshape(-1, x.shape[-1])
    while True:
        n = x.shape[0]
        groups = max(1, -(-n // 256))
        pad = np.zeros((groups * 256, x.shape[1]), np.float64)      # +0.0
        pad[:n] = x
        x = pad.reshape(groups, 256, -1)
        for _ in range(8):
            x = x[:, 0::2] + x[:, 1::2]
        x = x[:, 0]
        if groups == 1:
            return x[0]


def point_terms(verts, faces, unit_normal, q, face, mode):
    """the 29 float64 terms of every point -> [N,29]; rows without a match are +0.0"""
    V, Fc, U = _f32(verts), _faces(faces), _f32(unit_normal)
    n = q.shape[0]
    terms = np.zeros((n, SUMS), np.float64)
    hit = face >= 0
    if not hit.any():
        return terms
    qh, fh = q[hit], face[hit]
    with np.errstate(all="ignore"):
        a, b, c = (tuple(V[Fc[fh, s], t] - qh[:, t] for t in range(3)) for s in range(3))
        v, w, _ = closest(a, b, c)
        ab = tuple(b[k] - a[k] for k in range(3))
        ac = tuple(c[k] - a[k] for k in range(3))
        p = [(a[k] + ab[k] * v) + ac[k] * w for k in range(3)]
        one, zero = np.ones_like(p[0]), np.zeros_like(p[0])
        if mode == 0:
            normals = [(U[fh, 0], U[fh, 1], U[fh, 2])]
        else:
            normals = [(one, zero, zero), (zero, one, zero), (zero, zero, one)]
        total = None
        for nn in normals:
            r = (nn[0] * p[0] + nn[1] * p[1]) + nn[2] * p[2]
            J = [qh[:, 1] * nn[2] - qh[:, 2] * nn[1],
                 qh[:, 2] * nn[0] - qh[:, 0] * nn[2],
                 qh[:, 0] * nn[1] - qh[:, 1] * nn[0], nn[0], nn[1], nn[2]]
            assert r.dtype == F and all(j.dtype == F for j in J)
            J64 = [j.astype(np.float64) for j in J]
            r64 = r.astype(np.float64)
            row = np.stack([J64[i] * J64[j] for i, j in PAIRS] + [j * r64 for j in J64]
                           + [r64 * r64, np.ones_like(r64)], 1)
            total = row if total is None else total + row      # (x + y) + z
    terms[hit] = total
    return terms


def icp_sums(verts, faces, unit_normal, points, transform, max_dist, mode=0):
    """ucsa_icp_sums -> (sums float64 [29], face int32 [N], dist2 float32 [N], q float32 [N,3])"""
    q = transform_points(points, transform)
    face, dist2, _ = nearest_triangle(verts, faces, q, max_dist)
    terms = point_terms(verts, faces, unit_normal, q, face, mode)
    return tree_sum(terms), face, dist2, q


def register_points(points, verts, faces, unit_normal, init=None, max_dist=0.5, iterations=30,
                    mode=0, **solve):
    """The loop of utils.registration.register_points over this file's
    ``icp_sums``: every iteration's sums and the transforms -> (T, [sums ...])"""
    from ucsa_neural_rendering_amd.utils.registration import compose, solve_step
    T = np.eye(4) if init is None else np.array(init, np.float64)
    history = []
    for _ in range(iterations):
        sums = icp_sums(verts, faces, unit_normal, points, T, max_dist, mode)[0]
        history.append(sums)
        xi, _ = solve_step(sums, **solve)
        T = compose(T, xi)
    return T, history
