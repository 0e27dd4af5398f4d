"""numpy float32 restatement of the view-weight contracts in include/ucsa_hip.h
(``ucsa_depth_confidence`` and ``ucsa_tsdf_integrate_weighted``), written from
the header comments: the yardstick the GPU outputs are compared with, bit for
bit (test infrastructure).  ``confidence`` is a plain loop over the pixels and
``confidence_vec`` the same contract over whole arrays;
tests/test_weighted_fusion_cpu.py holds them to each other's bytes.
``integrate`` is tests/tsdf_numpy.py's ``integrate`` with the contract's changed
lines: a voxel sees its views one after the other."""
import numpy as np

from tests import tsdf_numpy as TN
from tests.depth_numpy import EDGE, GRAZING, MEASURED, NORMAL

F32 = np.float32


def confidence(points, normals, mask, sigma_depth, sigma_z2=0.0, cos_floor=0.1,
               reject=EDGE | GRAZING):
    """ucsa_depth_confidence -> weight [B,H,W] float32"""
    points, normals = np.asarray(points, F32), np.asarray(normals, F32)
    mask = np.asarray(mask, np.uint8)
    B, H, W = mask.shape
    sd, s2, cf, one = F32(sigma_depth), F32(sigma_z2), F32(cos_floor), F32(1.0)
    out = np.zeros((B, H, W), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(H):
                for j in range(W):
                    m = int(mask[b, i, j])
                    if not (m & MEASURED) or (m & int(reject)):
                        continue
                    p, n = points[b, i, j], normals[b, i, j]
                    z = p[2]
                    sigma = sd + s2 * (z * z)
                    s = sd / sigma
                    wz = s * s
                    wa = cf
                    if m & NORMAL:
                        dot = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
                        cosv = (-dot) / np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
                        # fminf(fmaxf(cosv, cos_floor), 1): a NaN cosv gives cos_floor
                        wa = np.fmin(np.fmax(cosv, cf), one)
                    out[b, i, j] = wz * wa
    return out


def confidence_vec(points, normals, mask, sigma_depth, sigma_z2=0.0, cos_floor=0.1,
                   reject=EDGE | GRAZING):
    points, normals = np.asarray(points, F32), np.asarray(normals, F32)
    mask = np.asarray(mask, np.uint8)
    sd, s2, cf, one = F32(sigma_depth), F32(sigma_z2), F32(cos_floor), F32(1.0)
    with np.errstate(all="ignore"):
        p0, p1, p2 = points[..., 0], points[..., 1], points[..., 2]
        n0, n1, n2 = normals[..., 0], normals[..., 1], normals[..., 2]
        sigma = sd + s2 * (p2 * p2)
        s = sd / sigma
        wz = s * s
        dot = (n0 * p0 + n1 * p1) + n2 * p2
        cosv = (-dot) / np.sqrt((p0 * p0 + p1 * p1) + p2 * p2)
        wa = np.where((mask & NORMAL) != 0, np.fmin(np.fmax(cosv, cf), one), cf).astype(F32)
        keep = ((mask & MEASURED) != 0) & ((mask & np.uint8(reject)) == 0)
        return np.where(keep, wz * wa, F32(0.0)).astype(F32)


def integrate(vol, depth, pixel_weight, poses, intrinsics, trunc, color=None, max_weight=65504.0,
              depth_min=1e-6, depth_max=3.0e38):
    """ucsa_tsdf_integrate_weighted.  In place; returns ``vol`` (tsdf_numpy.new_volume).
    depth, pixel_weight [B,H,W] f32, color [B,H,W,3] u8 or None, poses [B,4,4]."""
    depth = np.asarray(depth, F32)
    pixel_weight = np.asarray(pixel_weight, F32)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    B, H, W = depth.shape
    assert poses.shape[0] == B and pixel_weight.shape == (B, H, W)
    if (color is None) != (vol["rgb"] is None):
        raise ValueError("the colour volume and the colour frames come as a pair")
    if color is not None:
        color = np.asarray(color, np.uint8)
        assert color.shape == (B, H, W, 3)
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    trunc, max_weight = F32(trunc), F32(max_weight)
    dmin, dmax = F32(depth_min), F32(depth_max)
    px, py, pz = TN.voxel_centres(vol)
    tsdf, wgt, rgb = vol["tsdf"], vol["weight"], vol["rgb"]
    shape = tsdf.shape
    for b in range(B):
        P = poses[b]
        d0, d1, d2 = px - P[0, 3], py - P[1, 3], pz - P[2, 3]
        c = [np.broadcast_to((d0 * P[0, r] + d1 * P[1, r]) + d2 * P[2, r], shape)
             for r in range(3)]
        with np.errstate(all="ignore"):
            ok = c[2] > 0
            u = np.floor((fx * c[0]) / c[2] + cx)
            v = np.floor((fy * c[1]) / c[2] + cy)
            ok &= (u >= 0) & (u < F32(W)) & (v >= 0) & (v < F32(H))
            ui = np.where(ok, u, 0).astype(np.int64)
            vi = np.where(ok, v, 0).astype(np.int64)
            z = depth[b][vi, ui]
            ok &= np.isfinite(z) & (z >= dmin) & (z <= dmax)
            w = pixel_weight[b][vi, ui]
            ok &= (w > 0) & np.isfinite(w)
            sdf = z - c[2]
            ok &= ~(sdf < -trunc)
            x = np.minimum(F32(1.0), sdf / trunc)
            w1 = wgt + w
            new_t = (tsdf * wgt + x * w) / w1
            tsdf[ok] = new_t[ok]
            if rgb is not None:
                col = color[b][vi, ui].astype(F32)
                new_c = (rgb * wgt[..., None] + col * w[..., None]) / w1[..., None]
                rgb[ok] = new_c[ok]
            wgt[ok] = np.minimum(w1, max_weight)[ok]
    return vol
