"""numpy restatement of the scores of many rigid hypotheses against a TSDF volume
(csrc/tsdf_score.hip: ucsa_tsdf_score_transforms; ops.register.tsdf_scores) and
of the search around it (utils.registration.global_register_points_tsdf).

The sample is ``tsdf_register_numpy.sample``: vectorised float32, every
operation as the contract writes it.  The four numbers of a transform are exact
integers, so their sums are plain int64 sums: no tree.  The refinement is
``tsdf_register_numpy.register_points_tsdf``; ``rotation_set``, ``hypotheses``,
``surface_centroid``, ``compose`` and the solver are the host half of
``utils.registration``, as in ``tsdf_register_numpy``."""
import numpy as np

from tests import tsdf_register_numpy as TR

F = np.float32
SCALE = F(1048576.0)


def transform_rows(transforms):
    """[K,3,4], [K,4,4] or [K,12] -> float32 [K,12], the rows of [R | t]"""
    T = np.asarray(transforms)
    if T.ndim == 3:
        T = T[:, :3]
    return np.ascontiguousarray(T.astype(F).reshape(T.shape[0], 12))


def move(points, T12):
    """q_k = ((R[k][0]*x + R[k][1]*y) + R[k][2]*z) + t[k] in float32, T12 float32 [12]"""
    P = np.asarray(points, F).reshape(-1, 3)
    T = np.asarray(T12, F).reshape(3, 4)
    with np.errstate(all="ignore"):
        q = np.stack([((T[k, 0] * P[:, 0] + T[k, 1] * P[:, 1]) + T[k, 2] * P[:, 2]) + T[k, 3]
                      for k in range(3)], 1)
    assert q.dtype == F
    return q


def point_scores(vol, q, min_weight=1.0, max_tsdf=0.75):
    """per moved point -> (inlier bool [N], free bool [N], e int64 [N])"""
    s = TR.sample(vol, q, min_weight)
    with np.errstate(all="ignore"):
        a = np.abs(s["F"])
        inlier = s["inside"] & s["observed"] & (a <= F(max_tsdf))
        free = s["inside"] & s["observed"] & (s["F"] > F(max_tsdf))
        scaled = a * SCALE
        assert scaled.dtype == F
        e = np.where(inlier, np.rint(np.where(inlier, scaled, F(0))), F(0)).astype(np.int64)
    return inlier, free, e


def tsdf_scores(vol, points, transforms, min_weight=1.0, max_tsdf=0.75, chunk=1 << 21):
    """ucsa_tsdf_score_transforms -> int64 [K,4]: (inliers, free, sum e, sum e^2).
    The (transform, point) pairs are sampled ``chunk`` at a time."""
    T = transform_rows(transforms)
    P = np.asarray(points, F).reshape(-1, 3)
    K, n = T.shape[0], P.shape[0]
    out = np.zeros((K, 4), np.int64)
    if K == 0 or n == 0:
        return out
    per = max(1, int(chunk) // n)
    for k0 in range(0, K, per):
        k1 = min(K, k0 + per)
        q = _move_many(P, T[k0:k1])
        inlier, free, e = point_scores(vol, q, min_weight, max_tsdf)
        inlier, free, e = (x.reshape(k1 - k0, n) for x in (inlier, free, e))
        out[k0:k1, 0] = inlier.sum(1)
        out[k0:k1, 1] = free.sum(1)
        out[k0:k1, 2] = e.sum(1)
        out[k0:k1, 3] = (e * e).sum(1)
    return out


def _move_many(P, T):
    """``move`` for many transforms at once: float32 [K*N,3], transform-major"""
    with np.errstate(all="ignore"):
        x, y, z = (P[None, :, a] for a in range(3))
        q = np.stack([((T[:, 4 * k, None] * x + T[:, 4 * k + 1, None] * y)
                       + T[:, 4 * k + 2, None] * z) + T[:, 4 * k + 3, None] for k in range(3)], -1)
    assert q.dtype == F
    return q.reshape(-1, 3)


def rank_scores(scores):
    """best first: inliers - free descending, then sum e^2 ascending, then the index"""
    s = np.asarray(scores, np.int64).reshape(-1, 4)
    return sorted(range(s.shape[0]), key=lambda k: (-(int(s[k, 0]) - int(s[k, 1])), int(s[k, 3]), k))


def global_register_points_tsdf(points, vol, trunc, coarse=None, coarse_trunc=None,
                                n_rotations=4096, offsets=None, keep=16, max_tsdf=0.75,
                                coarse_iterations=10, fine_iterations=15, min_weight=1.0,
                                ambiguity_share=0.02, rotations=None):
    """utils.registration.global_register_points_tsdf over this file's
    ``tsdf_scores`` and the restated loop -> the same dict"""
    from ucsa_neural_rendering_amd.utils.registration import (hypotheses, is_ambiguous,
                                                              rotation_set, surface_centroid)
    P = np.asarray(points, F).reshape(-1, 3)
    if coarse is None:
        coarse, coarse_trunc = vol, trunc
    host = P.astype(np.float64)
    src_c = host[np.isfinite(host).all(1)].mean(0)
    R = rotation_set(n_rotations) if rotations is None else rotations
    H = hypotheses(R, src_c, surface_centroid(coarse, coarse_trunc, min_weight), offsets)
    first = tsdf_scores(coarse, P, H, min_weight, max_tsdf)
    refined = []
    for k in rank_scores(first)[:int(keep)]:
        out = TR.register_points_tsdf(P, coarse, coarse_trunc, init=H[k],
                                      iterations=coarse_iterations, min_weight=min_weight)
        out = TR.register_points_tsdf(P, vol, trunc, init=out["transform"],
                                      iterations=fine_iterations, min_weight=min_weight)
        refined.append((int(k), out))
    last = tsdf_scores(vol, P, np.stack([o["transform"] for _, o in refined]), min_weight,
                       max_tsdf)
    order = rank_scores(last)
    candidates = [{"index": refined[j][0], "transform": refined[j][1]["transform"],
                   "score": tuple(int(v) for v in last[j]),
                   "coarse_score": tuple(int(v) for v in first[refined[j][0]])} for j in order]
    result = dict(refined[int(order[0])][1])
    result.update(score=candidates[0]["score"], n_hypotheses=int(H.shape[0]),
                  candidates=candidates,
                  ambiguous=is_ambiguous(candidates, src_c, P.shape[0], float(trunc),
                                         ambiguity_share))
    return result
