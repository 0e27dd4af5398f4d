"""numpy float32 restatement of ``ucsa_mesh_voxelize_count`` / ``_fill``
(include/ucsa_hip.h), written from the header comment: the yardstick the GPU
masks are compared with, byte for byte (test infrastructure).  It knows nothing
of columns, offsets or searches: per face the box-axis predicate is evaluated on
every cell index of every axis, the cells that pass on all three form a box,
and the ten remaining axes are evaluated on that box as arrays.
``voxelize_brute`` is the definition as loops over (face, cell) pairs with
scalar fp32 arithmetic (``meets_scalar``) and pins the vectorised form;
``meets_scalar`` with ``K = 0`` is the test without its slack."""
import math

import numpy as np

F32 = np.float32
K_SLACK = 16                       # slack = K * 2^-24 * S
MAX_COORD = F32(2.0 ** 40)
_CYC = ((0, 1, 2), (1, 2, 0), (2, 0, 1))   # (a, b, c)


def default_cascade(bound):
    return 1 + math.ceil(math.log2(bound))


class Lattice:
    """the voxels of a tsdf_volume: dims, origin, spacing (scalar or 3), dilate"""
    ncas = 1

    def __init__(self, dims, origin, spacing, dilate=0.0):
        self.dims = tuple(int(d) for d in dims)
        self.origin = np.asarray(origin, F32)
        self.spacing = np.broadcast_to(np.asarray(spacing, F32), (3,))
        self.dilate = F32(dilate)
        self.shape = self.dims
        self.bmax = F32(0)
        for a in range(3):
            lo, hi = self.bounds(a, 0)
            self.bmax = max(self.bmax, abs(lo[0]), abs(hi[-1]))

    def bounds(self, a, cas):
        i = np.arange(self.dims[a]).astype(F32)
        p = (self.origin[a] + (i * self.spacing[a]).astype(F32)).astype(F32)
        h = F32(F32(0.5) * self.spacing[a])
        return ((p - h).astype(F32) - self.dilate).astype(F32), \
            ((p + h).astype(F32) + self.dilate).astype(F32)


class Cascade:
    """the marcher's cells: bound, cascade, H, dilate"""

    def __init__(self, bound, cascade=None, H=128, dilate=None):
        self.bound = F32(bound)
        self.ncas = default_cascade(bound) if cascade is None else int(cascade)
        self.H = int(H)
        self.dims = (self.H,) * 3
        self.dilate = F32(2.0 * min(1.0, float(bound)) / H) if dilate is None else F32(dilate)
        self.shape = (self.ncas,) + self.dims
        self.bmax = F32(min(F32(2.0) ** F32(self.ncas - 1), self.bound) + self.dilate)

    def bounds(self, a, cas):
        b = min(F32(2.0) ** F32(cas), self.bound)
        j = np.arange(self.H)
        Hf = F32(self.H)
        lo = (b * ((2 * j).astype(F32) / Hf - F32(1.0)).astype(F32)).astype(F32) - self.dilate
        hi = (b * ((2 * j + 2).astype(F32) / Hf - F32(1.0)).astype(F32)).astype(F32) + self.dilate
        return lo.astype(F32), hi.astype(F32)


def face_corners(verts, face):
    """-> p float32 [3 corners, 3 axes], or None when the face meets nothing
    because of its indices or corners"""
    V = verts.shape[0]
    idx = [int(i) for i in face]
    if any(i < 0 or i >= V for i in idx):
        return None
    p = np.asarray(verts, F32)[idx]
    if not (np.abs(p) <= MAX_COORD).all():      # NaN and inf fail
        return None
    return p


def face_terms(p, bmax, K=K_SLACK):
    """the per-face quantities of the contract"""
    S = max(F32(np.abs(p).max()), F32(bmax))
    slack = F32(F32(K * 2.0 ** -24) * S)
    e = np.stack([p[1] - p[0], p[2] - p[1], p[0] - p[2]]).astype(F32)   # [edge, axis]
    n = np.zeros(3, F32)
    for a, b, c in _CYC:
        n[a] = F32(e[0, b] * e[1, c]) - F32(e[0, c] * e[1, b])
    return {"p": p, "e": e, "n": n, "mn": p.min(0), "mx": p.max(0), "slack": slack}


def _rest_meets(t, lo, hi):
    """the ten axes that are not box axes; lo / hi: three float32 arrays, axis a
    shaped to broadcast along dimension a of the result"""
    s = t["slack"]
    c = [(F32(0.5) * (lo[a] + hi[a]).astype(F32)).astype(F32) for a in range(3)]
    g = [((F32(0.5) * (hi[a] - lo[a]).astype(F32)).astype(F32) + s).astype(F32) for a in range(3)]
    v = [[(t["p"][j, a] - c[a]).astype(F32) for a in range(3)] for j in range(3)]
    ok = True
    for a, b, cc in _CYC:
        for i in range(3):
            eb, ec = t["e"][i, b], t["e"][i, cc]
            q = [((eb * v[j][cc]).astype(F32) - (ec * v[j][b]).astype(F32)).astype(F32)
                 for j in range(3)]
            r = ((g[b] * abs(ec)).astype(F32) + (g[cc] * abs(eb)).astype(F32)).astype(F32)
            qmin = np.minimum(np.minimum(q[0], q[1]), q[2])
            qmax = np.maximum(np.maximum(q[0], q[1]), q[2])
            ok = ok & ~((qmin > r) | (qmax < -r))
    n = t["n"]
    d = [(((n[0] * v[j][0]).astype(F32) + (n[1] * v[j][1]).astype(F32)).astype(F32) +
          (n[2] * v[j][2]).astype(F32)).astype(F32) for j in range(3)]
    r = (((abs(n[0]) * g[0]).astype(F32) + (abs(n[1]) * g[1]).astype(F32)).astype(F32) +
         (abs(n[2]) * g[2]).astype(F32)).astype(F32)
    dmin = np.minimum(np.minimum(d[0], d[1]), d[2])
    dmax = np.maximum(np.maximum(d[0], d[1]), d[2])
    return ok & ~((dmin > r) | (dmax < -r))


def meets_scalar(p, lo, hi, bmax, K=K_SLACK, normal_corners=3):
    """meets(face, box) for one corner array p [3,3] and one box lo / hi [3],
    every operation a scalar fp32 one in the header's order.  ``normal_corners
    = 1`` is the textbook form of the normal axis, |n . v_0| <= |n| . g, which
    the contract does not use (it loses thin faces)"""
    p = np.asarray(p, F32)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    S = F32(bmax)
    for j in range(3):
        for a in range(3):
            S = max(S, abs(p[j, a]))
    slack = F32(F32(K * 2.0 ** -24) * S)
    for a in range(3):
        mn, mx = min(p[0, a], p[1, a], p[2, a]), max(p[0, a], p[1, a], p[2, a])
        if not (mn <= F32(hi[a] + slack) and mx >= F32(lo[a] - slack)):
            return False
    e = [[F32(p[1, a] - p[0, a]) for a in range(3)], [F32(p[2, a] - p[1, a]) for a in range(3)],
         [F32(p[0, a] - p[2, a]) for a in range(3)]]
    c = [F32(F32(0.5) * F32(lo[a] + hi[a])) for a in range(3)]
    g = [F32(F32(F32(0.5) * F32(hi[a] - lo[a])) + slack) for a in range(3)]
    v = [[F32(p[j, a] - c[a]) for a in range(3)] for j in range(3)]
    for a, b, cc in _CYC:
        for i in range(3):
            q = [F32(F32(e[i][b] * v[j][cc]) - F32(e[i][cc] * v[j][b])) for j in range(3)]
            r = F32(F32(g[b] * abs(e[i][cc])) + F32(g[cc] * abs(e[i][b])))
            if min(q) > r or max(q) < -r:
                return False
    n = [F32(F32(e[0][b] * e[1][cc]) - F32(e[0][cc] * e[1][b])) for a, b, cc in _CYC]
    d = [F32(F32(F32(n[0] * v[j][0]) + F32(n[1] * v[j][1])) + F32(n[2] * v[j][2]))
         for j in range(normal_corners)]
    r = F32(F32(F32(abs(n[0]) * g[0]) + F32(abs(n[1]) * g[1])) + F32(abs(n[2]) * g[2]))
    return not (min(d) > r or max(d) < -r)


def voxelize(verts, faces, fam, out=None):
    """-> uint8 mask of shape ``fam.shape``; ``out`` accumulates (met cells are
    set, every other byte is left alone)"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3)
    mask = np.zeros(fam.shape, np.uint8) if out is None else out
    view = mask.reshape((fam.ncas,) + fam.dims)
    bounds = [[fam.bounds(a, cas) for a in range(3)] for cas in range(fam.ncas)]
    with np.errstate(over="ignore", invalid="ignore"):
        for face in faces:
            p = face_corners(verts, face)
            if p is None:
                continue
            t = face_terms(p, fam.bmax)
            for cas in range(fam.ncas):
                sel = []
                for a in range(3):
                    lo, hi = bounds[cas][a]
                    ok = (t["mn"][a] <= (hi + t["slack"]).astype(F32)) & \
                        (t["mx"][a] >= (lo - t["slack"]).astype(F32))
                    sel.append(np.nonzero(ok)[0])
                if min(len(s) for s in sel) == 0:
                    continue
                lo3, hi3 = [], []
                for a in range(3):
                    shape = [1, 1, 1]
                    shape[a] = -1
                    lo3.append(bounds[cas][a][0][sel[a]].reshape(shape))
                    hi3.append(bounds[cas][a][1][sel[a]].reshape(shape))
                met = _rest_meets(t, lo3, hi3)
                sub = view[cas][np.ix_(*sel)]
                view[cas][np.ix_(*sel)] = np.where(met, np.uint8(1), sub)
    return mask


def voxelize_brute(verts, faces, fam):
    """the definition: loops over (face, cell) pairs; tiny cases only"""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    mask = np.zeros((fam.ncas,) + fam.dims, np.uint8)
    for face in np.asarray(faces).reshape(-1, 3):
        p = face_corners(verts, face)
        if p is None:
            continue
        for cas in range(fam.ncas):
            b = [fam.bounds(a, cas) for a in range(3)]
            for cell in np.ndindex(*fam.dims):
                if mask[(cas,) + cell]:
                    continue
                lo = [b[a][0][cell[a]] for a in range(3)]
                hi = [b[a][1][cell[a]] for a in range(3)]
                if meets_scalar(p, lo, hi, fam.bmax):
                    mask[(cas,) + cell] = 1
    return mask.reshape(fam.shape)


def iou_lattice(pred_verts, gt_verts, voxel, aabb=None):
    """the cubic lattice ``utils.mesh_eval.voxel_iou`` builds: the union box (or
    ``aabb`` [2,3]) padded by one voxel -> dims, origin (float32 [3])"""
    voxel = F32(voxel)
    if aabb is None:
        pts = np.concatenate([np.asarray(pred_verts, F32).reshape(-1, 3),
                              np.asarray(gt_verts, F32).reshape(-1, 3)])
        pts = pts[np.isfinite(pts).all(1)]
        box = np.stack([pts.min(0), pts.max(0)])
    else:
        box = np.asarray(aabb, F32).reshape(2, 3)
    lo = (box[0] - voxel).astype(F32)
    hi = (box[1] + voxel).astype(F32)
    dims = tuple(int(math.ceil(float(hi[a] - lo[a]) / float(voxel))) + 1 for a in range(3))
    return dims, lo


def voxel_iou(pred_verts, pred_faces, gt_verts, gt_faces, voxel, dilate=0.0, aabb=None):
    dims, origin = iou_lattice(pred_verts, gt_verts, voxel, aabb)
    fam = Lattice(dims, origin, voxel, dilate)
    a = voxelize(pred_verts, pred_faces, fam) != 0
    b = voxelize(gt_verts, gt_faces, fam) != 0
    inter, n_a, n_b = int((a & b).sum()), int(a.sum()), int(b.sum())
    union = n_a + n_b - inter
    return {"iou": inter / union if union else 1.0, "precision": inter / n_a if n_a else 1.0,
            "recall": inter / n_b if n_b else 1.0, "n_pred": n_a, "n_gt": n_b, "dims": dims,
            "voxel": float(F32(voxel))}
