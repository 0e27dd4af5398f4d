"""numpy restatement of the two weighted ICP steps (csrc/mesh_register.hip:
ucsa_projective_icp_sums_weighted, ucsa_tsdf_icp_sums_weighted;
ops.register.projective_sums_weighted, tsdf_sums_weighted) and of the host loops'
``robust`` / ``robust_scale`` / ``point_weight`` / ``view_weights`` keywords in
utils/registration.py.

The geometric half -- association, gates, the row (J, r) -- is
``projective_numpy.point_rows`` and ``tsdf_register_numpy.point_rows``, imported
as they are.  What is written here is the contract's second half: the weight
w = p * rho(|r|) in float32, one rounding per operation, the rows that count, the
scaling by sqrt(w), and the 29 float64 terms of the scaled floats summed by
``register_numpy.tree_sum``."""
import math

import numpy as np

from tests import projective_numpy as PJ
from tests import tsdf_register_numpy as TR
from tests import weighted_numpy as WN
from tests.register_numpy import transform_points, tree_sum

F = np.float32
KINDS = {"none": 0, "huber": 1, "tukey": 2}
EDGE, GRAZING, NORMAL = PJ.EDGE, PJ.GRAZING, PJ.NORMAL


def robust_weight(r, point_weight, robust="none", robust_scale=None):
    """w = p * rho(|r|) for every row -> float32 [N]; 0 where p is not finite and > 0.
    ``r`` float32 [N], ``point_weight`` float32 [N] or None (p = 1)."""
    r = np.asarray(r, F).reshape(-1)
    kind = KINDS[robust]
    with np.errstate(all="ignore"):
        a = np.abs(r)
        if kind == 0:
            rho = np.ones_like(a)
        elif kind == 1:
            k = F(robust_scale)
            rho = np.where(a <= k, F(1.0), k / a).astype(F)
        else:
            c = F(robust_scale)
            t = a / c
            u = F(1.0) - t * t
            rho = np.where(a < c, u * u, F(0.0)).astype(F)
        p = np.ones_like(a) if point_weight is None else np.asarray(point_weight, F).reshape(-1)
        assert p.shape == a.shape and rho.dtype == F
        usable = (p > 0) & np.isfinite(p)
        w = np.where(usable, p * rho, F(0.0)).astype(F)
    return w


def weighted_rows(matched, J, r, point_weight, robust, robust_scale):
    """the contract's second half -> (counts bool [N], J six float32 [N], r float32
    [N], weight float32 [N]): the scaled row where it counts, zeros elsewhere.
    ``J`` is a list of six arrays or [N,6]."""
    J = [np.asarray(J)[:, a] for a in range(6)] if not isinstance(J, list) else J
    with np.errstate(all="ignore"):
        w = robust_weight(r, point_weight, robust, robust_scale)
        counts = matched & (w > 0)
        s = np.sqrt(w)
        assert s.dtype == F
        Js = [np.where(counts, s * j, F(0.0)).astype(F) for j in J]
        rs = np.where(counts, s * r, F(0.0)).astype(F)
    return counts, Js, rs, np.where(counts, w, F(0.0)).astype(F)


def projective_sums_weighted(points, normals, tp, tn, tm, intrinsics, transform, max_dist,
                             min_cos=0.0, reject=EDGE | GRAZING, point_weight=None,
                             robust="none", robust_scale=None, rows=PJ.point_rows):
    """ucsa_projective_icp_sums_weighted -> (sums float64 [29], pixel int32 [N],
    residual float32 [N]: the unscaled r, NaN where unmatched, weight float32 [N])"""
    matched, J, r, pixel = rows(points, normals, tp, tn, tm, intrinsics, transform, max_dist,
                                min_cos, reject)
    counts, Js, rs, w = weighted_rows(matched, J, r, point_weight, robust, robust_scale)
    residual = np.where(matched, r, F(np.nan)).astype(F)
    return tree_sum(TR.point_terms(counts, Js, rs)), pixel, residual, w


def tsdf_sums_weighted(vol, points, transform, trunc, min_weight=1.0, max_tsdf=1.0,
                       point_weight=None, robust="none", robust_scale=None):
    """ucsa_tsdf_icp_sums_weighted -> (sums float64 [29], value float32 [N], matched
    uint8 [N], weight float32 [N])"""
    q = transform_points(points, transform)
    matched, J, r, value = TR.point_rows(vol, q, trunc, min_weight, max_tsdf)
    counts, Js, rs, w = weighted_rows(matched, J, r, point_weight, robust, robust_scale)
    return tree_sum(TR.point_terms(counts, Js, rs)), value, matched.astype(np.uint8), w


# ---------------------------------------------------------------------------
# the host loops of utils/registration.py with their new keywords
# ---------------------------------------------------------------------------
def source_weights(maps, reject, level_weight, view_weights, depth_filter):
    """utils.registration._source_weights -> float32 [N] or None"""
    if level_weight is None and view_weights is None:
        return None
    m = maps["mask"]
    keep = ((m & NORMAL) != 0) & ((m & np.uint8(reject)) == 0)
    if view_weights is not None:
        from ucsa_neural_rendering_amd.utils.depth_frontend import DepthFilter
        sd, s2 = view_weights.resolved(DepthFilter() if depth_filter is None else depth_filter)
        w = WN.confidence_vec(maps["points"][None], maps["normals"][None], m[None], sd, s2,
                              view_weights.cos_floor, reject)[0]
    else:
        w = np.asarray(level_weight, F)
        assert w.shape == m.shape
    return w[keep]


def register_frames(src_maps, dst_maps, intrinsics, init=None, iterations=(10, 5, 4),
                    max_dist=0.3, min_cos=0.8, reject=EDGE | GRAZING, rcond=1e-8, tol_rot=1e-6,
                    tol_trans=1e-6, robust="none", robust_scale=None, point_weight=None,
                    view_weights=None, depth_filter=None):
    """utils.registration.register_frames over this file's ``projective_sums_weighted``
    (always the weighted step: with the defaults its sums are the plain step's)"""
    from ucsa_neural_rendering_amd.utils.registration import (compose, normal_equations,
                                                              robust_schedule, solve_step)
    scales = robust_schedule(robust, robust_scale, len(iterations))
    if point_weight is not None and not isinstance(point_weight, (list, tuple)):
        point_weight = [point_weight]
    T = compose(np.eye(4) if init is None else np.asarray(init, np.float64), np.zeros(6))
    history, rank, done, converged, n_points = [], 0, 0, False, 0
    for level in reversed(range(len(iterations))):
        pts, nrm = PJ.source_rows(src_maps[level], reject)
        pw = source_weights(src_maps[level], reject,
                            None if point_weight is None else point_weight[level], view_weights,
                            depth_filter)
        dst = dst_maps[level]
        K = PJ.level_intrinsics(intrinsics, level)
        n_points, converged = pts.shape[0], False
        for _ in range(int(iterations[level])):
            sums = projective_sums_weighted(pts, nrm, dst["points"], dst["normals"], dst["mask"],
                                            K, T, max_dist, min_cos, reject, pw, robust,
                                            scales[level])[0]
            _, _, sse, count = normal_equations(sums)
            xi, rank = solve_step(sums, rcond)
            T = compose(T, xi)
            done += 1
            om, up = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
            history.append({"level": level, "matched": int(round(count)),
                            "rmse": math.sqrt(sse / count) if count > 0 else float("nan"),
                            "omega": om, "upsilon": up, "max_dist": float(max_dist),
                            "sums": sums, "robust": robust, "robust_scale": scales[level]})
            if count > 0 and om <= tol_rot and up <= tol_trans:
                converged = True
                break
    last = history[-1] if history else {"matched": 0, "rmse": float("nan")}
    return {"transform": T, "rmse": last["rmse"], "matched": last["matched"], "rank": rank,
            "iterations": done, "converged": converged, "history": history,
            "n_points": int(n_points)}


def odometry(depths, intrinsics, flt=None, filtered=False, iterations=(10, 5, 4),
             min_matched=0.25, **kw):
    """utils.registration.odometry over this file's ``register_frames`` -> (poses
    [N,4,4] float64, records, fallbacks)"""
    levels = len(iterations)
    if kw.get("view_weights") is not None:
        kw.setdefault("depth_filter", flt)
    maps = [PJ.frame_maps(d, intrinsics, flt, levels, filtered) for d in depths]
    poses, records, fallbacks = [np.eye(4)], [None], 0
    for i in range(1, len(maps)):
        out = register_frames(maps[i], maps[i - 1], intrinsics, iterations=iterations, **kw)
        share = out["matched"] / out["n_points"] if out["n_points"] else 0.0
        fallback = bool(out["rank"] < 6 or share < min_matched)
        fallbacks += fallback
        poses.append(poses[-1] @ (np.eye(4) if fallback else out["transform"]))
        records.append({"matched": share, "rmse": out["rmse"], "rank": out["rank"],
                        "iterations": out["iterations"], "fallback": fallback})
    return np.stack(poses), records, fallbacks


def register_points_tsdf(points, vol, trunc, init=None, iterations=30, min_weight=1.0,
                         max_tsdf=1.0, max_tsdf_schedule=None, tol_rot=1e-6, tol_trans=1e-6,
                         rcond=1e-8, robust="none", robust_scale=None, point_weight=None):
    """utils.registration.register_points_tsdf over this file's ``tsdf_sums_weighted``"""
    from ucsa_neural_rendering_amd.utils.registration import (compose, normal_equations,
                                                              robust_schedule, solve_step)
    T = compose(np.eye(4) if init is None else np.asarray(init, np.float64), np.zeros(6))
    schedule = [float(max_tsdf)] if max_tsdf_schedule is None else \
        [float(m) for m in max_tsdf_schedule]
    scales = robust_schedule(robust, robust_scale)
    history, rank, converged, done = [], 0, False, 0
    for k in range(int(iterations)):
        mt = schedule[min(k, len(schedule) - 1)]
        sc = scales[min(k, len(scales) - 1)]
        sums = tsdf_sums_weighted(vol, points, T, trunc, min_weight, mt, point_weight, robust,
                                  sc)[0]
        _, _, sse, count = normal_equations(sums)
        xi, rank = solve_step(sums, rcond)
        T = compose(T, xi)
        done = k + 1
        om, up = float(np.linalg.norm(xi[:3])), float(np.linalg.norm(xi[3:]))
        history.append({"matched": int(round(count)),
                        "rmse": math.sqrt(sse / count) if count > 0 else float("nan"),
                        "omega": om, "upsilon": up, "max_tsdf": mt, "sums": sums,
                        "robust": robust, "robust_scale": sc})
        if count > 0 and om <= tol_rot and up <= tol_trans:
            converged = True
            break
    last = history[-1] if history else {"matched": 0, "rmse": float("nan")}
    return {"transform": T, "rmse": last["rmse"], "matched": last["matched"], "rank": rank,
            "iterations": done, "converged": converged, "history": history,
            "n_points": int(np.asarray(points).reshape(-1, 3).shape[0])}
