"""numpy float32 restatement of ``ucsa_tsdf_occupancy`` (include/ucsa_hip.h),
written from the header comment: the yardstick the GPU masks are compared with,
byte for byte (test infrastructure).  It knows nothing of packed words, waves
or searches: per axis the contract's own predicate gives a boolean [H, n]
matrix "voxel i meets cell j", and the OR over a cell's box of voxels is three
range-ORs applied one after the other.  ``occupancy_brute`` loops over (cell,
voxel) pairs for tiny cases and pins the separable form."""
import math

import numpy as np

F32 = np.float32


def default_cascade(bound):
    return 1 + math.ceil(math.log2(bound))


def voxel_axis(origin, spacing, n):
    """p [n] fp32 = origin + float(i) * spacing, and h = 0.5f * spacing"""
    p = (F32(origin) + np.arange(n).astype(F32) * F32(spacing)).astype(F32)
    return p, F32(F32(0.5) * F32(spacing))


def cell_axis(cas, H, bound, dilate):
    """lo, hi [H] fp32 of the dilated cells of cascade ``cas`` on one axis"""
    b = min(F32(2.0) ** F32(cas), F32(bound))
    j = np.arange(H)
    Hf = F32(H)
    lo = (b * ((2 * j).astype(F32) / Hf - F32(1.0)).astype(F32)).astype(F32) - F32(dilate)
    hi = (b * ((2 * j + 2).astype(F32) / Hf - F32(1.0)).astype(F32)).astype(F32) + F32(dilate)
    return lo.astype(F32), hi.astype(F32)


def axis_overlap(origin, spacing, n, cas, H, bound, dilate):
    """-> meets bool [H, n], outside bool [H] for one axis of one cascade"""
    p, h = voxel_axis(origin, spacing, n)
    lo, hi = cell_axis(cas, H, bound, dilate)
    top, bottom = (p + h).astype(F32), (p - h).astype(F32)
    meets = (top[None, :] >= lo[:, None]) & (bottom[None, :] <= hi[:, None])
    outside = (lo < bottom[0]) | (hi > top[-1])
    return meets, outside


def not_free(tsdf, weight, min_weight=1.0, free_tsdf=1.0, unknown="keep"):
    """bool [nx,ny,nz]: the voxels that block carving"""
    tsdf, weight = np.asarray(tsdf, F32), np.asarray(weight, F32)
    with np.errstate(invalid="ignore"):
        seen = weight >= F32(min_weight)
        free = seen & (tsdf >= F32(free_tsdf))
    if unknown == "empty":
        free = free | ~seen
    elif unknown != "keep":
        raise ValueError(unknown)
    return ~free


def _range_or(A, x, axis):
    """OR over the voxels of ``axis`` that each cell meets: A bool [H, n],
    x bool [...] with n along ``axis`` -> bool with H there (counts stay exact
    in fp32: n < 2^24)"""
    x = np.moveaxis(x, axis, 0)
    y = A.astype(F32) @ x.reshape(x.shape[0], -1).astype(F32)
    return np.moveaxis((y > 0).reshape((A.shape[0],) + x.shape[1:]), 0, axis)


def occupancy(tsdf, weight, origin, spacing, bound, cascade=None, H=128, dilate=None,
              min_weight=1.0, free_tsdf=1.0, unknown="keep"):
    """-> uint8 [cascade,H,H,H]; the defaults are ``ops.tsdf_occupancy``'s"""
    spacing = np.broadcast_to(np.asarray(spacing, F32), (3,))
    origin = np.asarray(origin, F32)
    cascade = default_cascade(bound) if cascade is None else int(cascade)
    dilate = F32(spacing.max()) if dilate is None else F32(dilate)
    blocked = not_free(tsdf, weight, min_weight, free_tsdf, unknown)
    dims = blocked.shape
    out = np.zeros((cascade, H, H, H), np.uint8)
    for cas in range(cascade):
        ax = [axis_overlap(origin[a], spacing[a], dims[a], cas, H, bound, dilate)
              for a in range(3)]
        kept = blocked
        for a in range(3):
            kept = _range_or(ax[a][0], kept, a)
        if unknown == "keep":
            kept = kept | ax[0][1][:, None, None] | ax[1][1][None, :, None] | \
                ax[2][1][None, None, :]
        out[cas] = kept
    return out


def occupancy_brute(tsdf, weight, origin, spacing, bound, cascade, H, dilate, min_weight=1.0,
                    free_tsdf=1.0, unknown="keep"):
    """The definition as loops over (cell, voxel) pairs with scalar fp32
    arithmetic; tiny cases only."""
    spacing = np.broadcast_to(np.asarray(spacing, F32), (3,))
    origin = np.asarray(origin, F32)
    tsdf, weight = np.asarray(tsdf, F32), np.asarray(weight, F32)
    dims = tsdf.shape
    one, half = F32(1.0), F32(0.5)
    out = np.zeros((cascade, H, H, H), np.uint8)

    def free(i, j, k):
        t, w = tsdf[i, j, k], weight[i, j, k]
        seen = bool(w >= F32(min_weight))
        if seen and bool(t >= F32(free_tsdf)):
            return True
        return unknown == "empty" and not seen

    for cas in range(cascade):
        b = min(F32(2 ** cas), F32(bound))
        for cell in np.ndindex(H, H, H):
            lo = [F32(F32(b * F32(F32(F32(2 * cell[a]) / F32(H)) - one)) - F32(dilate))
                  for a in range(3)]
            hi = [F32(F32(b * F32(F32(F32(2 * cell[a] + 2) / F32(H)) - one)) + F32(dilate))
                  for a in range(3)]
            keep = False
            for a in range(3):
                h = F32(half * spacing[a])
                first = F32(origin[a] + F32(F32(0) * spacing[a]))
                last = F32(origin[a] + F32(F32(dims[a] - 1) * spacing[a]))
                if unknown == "keep" and (lo[a] < F32(first - h) or hi[a] > F32(last + h)):
                    keep = True
            if not keep:
                for vox in np.ndindex(*dims):
                    meets = True
                    for a in range(3):
                        h = F32(half * spacing[a])
                        p = F32(origin[a] + F32(F32(vox[a]) * spacing[a]))
                        if not (F32(p + h) >= lo[a] and F32(p - h) <= hi[a]):
                            meets = False
                            break
                    if meets and not free(*vox):
                        keep = True
                        break
            out[(cas,) + cell] = keep
    return out


def marcher_cell(points, bound, cascade, H):
    """The cell the marcher's lookup (Marcher::look, oracle/raymarch.c) maps
    points [N,3] to, in fp32: -> level [N], idx [N,3] int."""
    p = np.clip(np.asarray(points, F32), F32(-bound), F32(bound))
    mx = np.abs(p).max(1)
    _, e = np.frexp(mx)
    level = np.minimum(F32(cascade - 1), np.maximum(F32(0), e.astype(F32))).astype(np.int64)
    mip = np.minimum(np.exp2(level.astype(F32)), F32(bound)).astype(F32)
    r = (F32(1.0) / mip).astype(F32)
    q = (F32(0.5) * ((p * r[:, None]).astype(F32) + F32(1.0))).astype(F32) * F32(H)
    idx = np.clip(q.astype(F32), F32(0), F32(H - 1)).astype(np.int64)
    return level, idx


def points_kept(mask, points, bound):
    """bool [N]: the marcher's cell of each point is a kept cell"""
    cascade, H = mask.shape[0], mask.shape[1]
    level, idx = marcher_cell(points, bound, cascade, H)
    return mask[level, idx[:, 0], idx[:, 1], idx[:, 2]] != 0
