"""Vectorised numpy restatement of the mesh-rasterization contract of
``ucsa_raster_setup`` / ``ucsa_raster_draw`` (include/ucsa_hip.h): the
yardstick the GPU kernels are compared with, bit for bit (test
infrastructure).  Every float operation is a float32 numpy operation in the
header's order; clipping (rare: faces crossing the near plane or the guard
band) runs face by face on float32 scalars."""
import numpy as np

F32 = np.float32
GUARD = F32(65536.0)
CLAMP = F32(2097152.0)
TILE = 16
MAXP = 8
WORK = 12
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera_points(verts, pose):
    """verts [V,3] -> camera coordinates [V,3] f32: c_r = (d0*R0r + d1*R1r) + d2*R2r,
    d = p - t."""
    v = np.asarray(verts, F32)
    P = np.asarray(pose, F32)
    d0, d1, d2 = v[:, 0] - P[0, 3], v[:, 1] - P[1, 3], v[:, 2] - P[2, 3]
    return np.stack([(d0 * P[0, r] + d1 * P[1, r]) + d2 * P[2, r] for r in range(3)], 1)


class _Cam:
    def __init__(self, intrinsics, H, W, near):
        fx, fy, cx, cy = (F32(v) for v in intrinsics)
        self.fx, self.fy, self.cx, self.cy, self.near = fx, fy, cx, cy, F32(near)
        self.kL = cx + GUARD
        self.kR = (F32(W) + GUARD) - cx
        self.kT = cy + GUARD
        self.kB = (F32(H) + GUARD) - cy
        self.H, self.W = H, W

    def plane(self, p, x, y, z):
        if p == 0:
            return z - self.near
        if p == 1:
            return x * self.fx + z * self.kL
        if p == 2:
            return z * self.kR - x * self.fx
        if p == 3:
            return y * self.fy + z * self.kT
        return z * self.kB - y * self.fy


def _clip(k, c, idx):
    """Sutherland-Hodgman of one face (c [3,3] f32 corners, idx its vertex
    indices) -> list of (x, y, z) float32 or None."""
    poly = [(c[q, 0], c[q, 1], c[q, 2], 1 << q) for q in range(3)]
    for p in range(5):
        if not poly:
            break
        out = []
        n = len(poly)
        for i in range(n):
            A, B = poly[i], poly[(i + 1) % n]
            sA, sB = k.plane(p, *A[:3]), k.plane(p, *B[:3])
            inA, inB = bool(sA >= 0), bool(sB >= 0)
            if inA:
                out.append(A)
            if inA != inB:
                um = A[3] | B[3]
                if bin(um).count("1") == 2:
                    a = (um & -um).bit_length() - 1
                    b = (um & (um - 1)).bit_length() - 1
                    lo, hi = (a, b) if idx[a] <= idx[b] else (b, a)
                    Pp, Q = c[lo], c[hi]
                    sP, sQ = k.plane(p, *Pp), k.plane(p, *Q)
                    om = um
                else:
                    Pp, Q = A[:3], B[:3]
                    sP, sQ = sA, sB
                    om = 7
                t = sP / (sP - sQ)
                if not (t >= 0):
                    t = F32(0)
                if t > 1:
                    t = F32(1)
                out.append(tuple(Pp[q] + t * (Q[q] - Pp[q]) for q in range(3)) + (om,))
        if len(out) > WORK:
            return None
        poly = out
    if len(poly) < 3 or len(poly) > MAXP:
        return None
    return [v[:3] for v in poly]


def _snap(k, x, y, z):
    u = k.fx * (x / z) + k.cx
    v = k.fy * (y / z) + k.cy
    u = np.where(~(u >= -CLAMP), -CLAMP, u)
    u = np.where(u > CLAMP, CLAMP, u)
    v = np.where(~(v >= -CLAMP), -CLAMP, v)
    v = np.where(v > CLAMP, CLAMP, v)
    return (np.rint(u * F32(256)).astype(np.int64), np.rint(v * F32(256)).astype(np.int64))


def _edge(px, py, qx, qy, x, y):
    return (qx - px) * (y - py) - (qy - py) * (x - px)


def _in_edge(px, py, qx, qy, x, y):
    e = _edge(px, py, qx, qy, x, y)
    dy, dx = qy - py, qx - px
    return (e > 0) | ((e == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def setup_view(verts, faces, pose, k):
    """The records of one view: dict of per-face arrays (n == 0: nothing)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    F, V = faces.shape[0], verts.shape[0]
    cam = camera_points(verts, pose)
    ok = ((faces >= 0) & (faces < V)).all(1)
    fi = np.where(ok[:, None], faces, 0)
    C = cam[fi]  # [F,3,3]
    ok &= np.isfinite(C).all((1, 2))
    s = np.stack([k.plane(p, C[..., 0], C[..., 1], C[..., 2]) for p in range(5)])
    ins = s >= 0
    ok &= ~(~ins).all(2).any(0)
    all_in = ins.all((0, 2))
    px = np.zeros((F, MAXP), np.int64)
    py = np.zeros((F, MAXP), np.int64)
    n = np.zeros(F, np.int64)
    zmin = np.zeros(F, F32)
    zmax = np.zeros(F, F32)
    fast = ok & all_in
    X, Y = _snap(k, C[fast, :, 0], C[fast, :, 1], C[fast, :, 2])
    px[fast, :3], py[fast, :3], n[fast] = X, Y, 3
    zmin[fast] = C[fast, :, 2].min(1)
    zmax[fast] = C[fast, :, 2].max(1)
    with np.errstate(all="ignore"):
        for f in np.nonzero(ok & ~all_in)[0]:
            poly = _clip(k, C[f], fi[f])
            if poly is None:
                continue
            P = np.array(poly, F32)
            X, Y = _snap(k, P[:, 0], P[:, 1], P[:, 2])
            m = P.shape[0]
            px[f, :m], py[f, :m], n[f] = X, Y, m
            zmin[f], zmax[f] = P[:, 2].min(), P[:, 2].max()
    flags = np.zeros(F, np.int64)
    for t in range(MAXP - 2):
        area = _edge(px[:, 0], py[:, 0], px[:, t + 1], py[:, t + 1], px[:, t + 2], py[:, t + 2])
        has = n > t + 2
        flags |= ((has & (area != 0)).astype(np.int64) << (2 * t))
        flags |= ((has & (area < 0)).astype(np.int64) << (2 * t + 1))
    big = np.int64(1) << 40
    xs = np.where(np.arange(MAXP)[None] < n[:, None], px, big)
    ys = np.where(np.arange(MAXP)[None] < n[:, None], py, big)
    x0 = np.maximum((xs.min(1) - 128 + 255) >> 8, 0)
    y0 = np.maximum((ys.min(1) - 128 + 255) >> 8, 0)
    xs = np.where(np.arange(MAXP)[None] < n[:, None], px, -big)
    ys = np.where(np.arange(MAXP)[None] < n[:, None], py, -big)
    x1 = np.minimum((xs.max(1) - 128) >> 8, k.W - 1)
    y1 = np.minimum((ys.max(1) - 128) >> 8, k.H - 1)
    live = (n >= 3) & (flags != 0) & (x0 <= x1) & (y0 <= y1)
    e1 = [C[:, 1, q] - C[:, 0, q] for q in range(3)]
    e2 = [C[:, 2, q] - C[:, 0, q] for q in range(3)]
    nn = _cross(e1, e2)
    nc0 = _dot(nn, [C[:, 0, q] for q in range(3)])
    zlo = np.where(zmin < k.near, k.near, zmin)
    zhi = np.where(zmax < zlo, zlo, zmax)
    return dict(live=live, n=n, px=px, py=py, flags=flags, x0=x0, x1=x1, y0=y0, y1=y1,
                nn=nn, nc0=nc0, zlo=zlo, zhi=zhi, C=C, fi=fi)


def _rays(k, xs, ys):
    dx = ((xs.astype(F32) + F32(0.5)) - k.cx) / k.fx
    dy = ((ys.astype(F32) + F32(0.5)) - k.cy) / k.fy
    return dx, dy


def draw_view(rec, k, chunk=1 << 22):
    """-> best key per pixel [H*W] uint64."""
    H, W = k.H, k.W
    best = np.full(H * W, EMPTY, np.uint64)
    ids = np.nonzero(rec["live"])[0]
    if ids.size == 0:
        return best
    bw = rec["x1"][ids] - rec["x0"][ids] + 1
    area = bw * (rec["y1"][ids] - rec["y0"][ids] + 1)
    ends = np.cumsum(area)
    a = 0
    while a < ids.size:
        b = int(np.searchsorted(ends, (ends[a - 1] if a else 0) + chunk, side="right"))
        b = max(b, a + 1)
        sel, sa, sw = ids[a:b], area[a:b], bw[a:b]
        rep = np.repeat(np.arange(sel.size), sa)
        start = np.concatenate([[0], np.cumsum(sa)[:-1]])
        loc = np.arange(rep.size) - start[rep]
        f = sel[rep]
        xs = rec["x0"][f] + loc % sw[rep]
        ys = rec["y0"][f] + loc // sw[rep]
        PX, PY = xs * 256 + 128, ys * 256 + 128
        px, py, fl = rec["px"][f], rec["py"][f], rec["flags"][f]
        cov = np.zeros(f.size, bool)
        for t in range(MAXP - 2):
            ft = (fl >> (2 * t)) & 3
            on = (ft & 1) != 0
            if not on.any():
                continue
            ax, ay = px[:, 0], py[:, 0]
            sw_ = (ft & 2) != 0
            bx = np.where(sw_, px[:, t + 2], px[:, t + 1])
            by = np.where(sw_, py[:, t + 2], py[:, t + 1])
            cx = np.where(sw_, px[:, t + 1], px[:, t + 2])
            cy = np.where(sw_, py[:, t + 1], py[:, t + 2])
            cov |= on & _in_edge(ax, ay, bx, by, PX, PY) & _in_edge(bx, by, cx, cy, PX, PY) \
                & _in_edge(cx, cy, ax, ay, PX, PY)
        f, xs, ys = f[cov], xs[cov], ys[cov]
        dx, dy = _rays(k, xs, ys)
        with np.errstate(all="ignore"):
            z = rec["nc0"][f] / ((rec["nn"][0][f] * dx + rec["nn"][1][f] * dy) + rec["nn"][2][f])
        zlo, zhi = rec["zlo"][f], rec["zhi"][f]
        z = np.where(np.isfinite(z), z, zhi)
        z = np.where(z < zlo, zlo, z)
        z = np.where(z > zhi, zhi, z).astype(F32)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | f.astype(np.uint64)
        np.minimum.at(best, ys * W + xs, key)
        a = b
    return best


def resolve_view(best, rec, k, vertex_labels=None, vertex_rgb=None):
    H, W = k.H, k.W
    tri = np.full(H * W, -1, np.int32)
    depth = np.zeros(H * W, F32)
    label = np.zeros(H * W, np.int32)
    rgb = np.zeros((H * W, 3), F32) if vertex_rgb is not None else None
    pix = np.nonzero(best != EMPTY)[0]
    f = (best[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    z = (best[pix] >> np.uint64(32)).astype(np.uint32).view(F32)
    dx, dy = _rays(k, pix % W, pix // W)
    C = rec["C"][f]
    c0 = [C[:, 0, q] for q in range(3)]
    e1 = [C[:, 1, q] - C[:, 0, q] for q in range(3)]
    e2 = [C[:, 2, q] - C[:, 0, q] for q in range(3)]
    nn = _cross(e1, e2)
    q = [z * dx - c0[0], z * dy - c0[1], z - c0[2]]
    with np.errstate(all="ignore"):
        nsq = _dot(nn, nn)
        w1 = _dot(nn, _cross(q, e2)) / nsq
        w2 = _dot(nn, _cross(e1, q)) / nsq
        w0 = (F32(1) - w1) - w2
    bad = ~(np.isfinite(w0) & np.isfinite(w1) & np.isfinite(w2))
    w0 = np.where(bad, F32(1), w0)
    w1 = np.where(bad, F32(0), w1)
    w2 = np.where(bad, F32(0), w2)
    corner = np.where((w0 >= w1) & (w0 >= w2), 0, np.where(w1 >= w2, 1, 2))
    idx = rec["fi"][f]
    tri[pix] = f
    depth[pix] = z
    if vertex_labels is not None:
        label[pix] = np.asarray(vertex_labels, np.int32)[idx[np.arange(f.size), corner]]
    if rgb is not None:
        col = np.asarray(vertex_rgb, F32)
        r0, r1, r2 = col[idx[:, 0]], col[idx[:, 1]], col[idx[:, 2]]
        rgb[pix] = (w0[:, None] * r0 + w1[:, None] * r1) + w2[:, None] * r2
    return tri, depth, label, rgb


def rasterize(verts, faces, poses, intrinsics, H, W, near, vertex_labels=None,
              vertex_rgb=None):
    """-> dict tri_id [B,H,W] int32, depth f32, label int32, rgb [B,H,W,3] f32
    (only with vertex_rgb): the bits of ops.rasterize_mesh."""
    verts = np.asarray(verts, F32).reshape(-1, 3)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    k = _Cam(intrinsics, H, W, near)
    outs = {"tri_id": [], "depth": [], "label": [], "rgb": []}
    for b in range(poses.shape[0]):
        rec = setup_view(verts, faces, poses[b], k)
        best = draw_view(rec, k)
        tri, dep, lab, rgb = resolve_view(best, rec, k, vertex_labels, vertex_rgb)
        outs["tri_id"].append(tri.reshape(H, W))
        outs["depth"].append(dep.reshape(H, W))
        outs["label"].append(lab.reshape(H, W))
        if rgb is not None:
            outs["rgb"].append(rgb.reshape(H, W, 3))
    res = {key: np.stack(v) for key, v in outs.items() if v}
    return res
