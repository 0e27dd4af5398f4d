"""numpy float32 restatement of the voxel-map contracts of include/ucsa_hip.h:
``ucsa_tsdf_vote`` (per-voxel class votes), ``ucsa_voxel_label_resolve`` and
``ucsa_tsdf_raycast`` (the ray-caster over the TSDF volume, plain and with the
marked bricks), written from the header comments: the yardstick the GPU outputs
are compared with, bit for bit (test infrastructure).  Vectorised over voxels
and rays, a loop over views and over the sample index k; it knows nothing of
launches, patches or waves."""
import numpy as np

from tests import tsdf_numpy as TN

F32 = np.float32
MARK_EPS = F32(2.0 ** -16)
BRICK = 8
MAXK = 1 << 20


def new_votes(dims, n_classes):
    assert 1 <= n_classes <= 255
    return np.zeros((n_classes + 1,) + tuple(int(d) for d in dims), np.uint16)


def vote(votes, vol, depth, pred, poses, intrinsics, trunc, depth_min=1e-6, depth_max=3.0e38):
    """In place; returns ``votes``.  vol: origin / spacing / the dims of
    ``tsdf`` only (the TSDF state is not read)."""
    depth = np.asarray(depth, F32)
    pred = np.asarray(pred, np.uint8)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    B, H, W = depth.shape
    assert poses.shape[0] == B and pred.shape == depth.shape
    Cn = votes.shape[0] - 1
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    trunc, dmin, dmax = F32(trunc), F32(depth_min), F32(depth_max)
    px, py, pz = TN.voxel_centres(vol)
    shape = votes.shape[1:]
    assert shape == vol["tsdf"].shape
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
            sdf = z - c[2]
            ok &= (sdf >= -trunc) & (sdf <= trunc)
        cls = pred[b][vi, ui].astype(np.int64)
        ok &= (cls >= 1) & (cls <= Cn)
        i, j, k = np.nonzero(ok)
        cl = cls[i, j, k]
        cur = votes[cl, i, j, k].astype(np.int64)  # (class, voxel) pairs are distinct
        votes[cl, i, j, k] = np.minimum(cur + 1, 65535).astype(np.uint16)
    return votes


def resolve(votes, min_votes=1):
    """-> label [nx,ny,nz] uint8, total uint32, winner uint32"""
    s = votes[1:].astype(np.uint32)
    total = s.sum(0, dtype=np.uint32)
    winner = s.max(0)
    arg = (np.argmax(s, 0) + 1).astype(np.uint8)  # the first maximum: the lowest class
    label = np.where(total >= np.uint32(min_votes), arg, np.uint8(0)).astype(np.uint8)
    return label, total, winner


def brick_marks(vol, min_weight=1.0):
    """[nbx,nby,nbz] bool: bricks of 8^3 cells that hold a cell with eight valid
    corners, one of them <= 2^-16"""
    valid = vol["weight"] >= F32(min_weight)
    low = vol["tsdf"] <= MARK_EPS
    nx, ny, nz = valid.shape
    whole = np.ones((nx - 1, ny - 1, nz - 1), bool)
    any_low = np.zeros((nx - 1, ny - 1, nz - 1), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                sl = (slice(di, nx - 1 + di), slice(dj, ny - 1 + dj), slice(dk, nz - 1 + dk))
                whole &= valid[sl]
                any_low |= low[sl]
    cell = whole & any_low
    nb = [-(-(n - 1) // BRICK) for n in (nx, ny, nz)]
    pad = np.zeros([b * BRICK for b in nb], bool)
    pad[:nx - 1, :ny - 1, :nz - 1] = cell
    return pad.reshape(nb[0], BRICK, nb[1], BRICK, nb[2], BRICK).any((1, 3, 5))


def _lerp(x, y, f):
    return x + f * (y - x)


class _Cells:
    """cells and clamped fractions of the points g(z) of some rays"""

    def __init__(self, dims, q0, qd, z):
        self.c, self.f, self.g = [], [], []
        for a in range(3):
            g = q0[a] + z * qd[a]
            fl = np.clip(np.floor(g), F32(0), F32(dims[a] - 2))
            self.g.append(g)
            self.c.append(fl.astype(np.int64))
            self.f.append(np.minimum(np.maximum(g - fl, F32(0)), F32(1)))

    def corners(self, arr):
        """[8, n] (or [8, n, ch]): v[4i + 2j + k]"""
        c = self.c
        return np.stack([arr[c[0] + i, c[1] + j, c[2] + k]
                         for i in (0, 1) for j in (0, 1) for k in (0, 1)])

    def parts(self, v):
        f = self.f
        if v.ndim == 3:
            f = [x[:, None] for x in f]
        c00, c01 = _lerp(v[0], v[1], f[2]), _lerp(v[2], v[3], f[2])
        c10, c11 = _lerp(v[4], v[5], f[2]), _lerp(v[6], v[7], f[2])
        c0, c1 = _lerp(c00, c01, f[1]), _lerp(c10, c11, f[1])
        return c00, c01, c10, c11, c0, c1, f

    def trilerp(self, v):
        *_, c0, c1, f = self.parts(v)
        return _lerp(c0, c1, f[0])

    def sample(self, vol, min_weight):
        valid = (self.corners(vol["weight"]) >= min_weight).all(0)
        return self.trilerp(self.corners(vol["tsdf"])), valid

    def marked(self, marks):
        return marks[self.c[0] // BRICK, self.c[1] // BRICK, self.c[2] // BRICK]


def raycast(vol, poses, intrinsics, H, W, near, far, trunc, step=None, min_weight=1.0,
            voxel_labels=None, skip=False, stats=None):
    """-> dict: depth [B,H,W] f32, voxel_id int32, normal [B,H,W,3] f32, rgb
    [B,H,W,3] f32 if the volume has colour, label int32 if voxel_labels.
    ``skip``: evaluate index k only if sample k or k+1 lies in a marked brick.
    ``stats``: a dict that receives the number of evaluated indices."""
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    B = poses.shape[0]
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    near, far, trunc = F32(near), F32(far), F32(trunc)
    step = F32(0.5) * trunc if step is None else F32(step)
    assert near > 0 and far >= near and 0 < step < trunc
    min_weight = F32(min_weight)
    dims = vol["tsdf"].shape
    o, h = np.asarray(vol["origin"], F32), np.asarray(vol["spacing"], F32)
    marks = brick_marks(vol, min_weight) if skip else None
    ys, xs = np.mgrid[0:H, 0:W]
    d0 = (((xs.astype(F32) + F32(0.5)) - cx) / fx).reshape(-1)
    d1 = (((ys.astype(F32) + F32(0.5)) - cy) / fy).reshape(-1)
    dz_all = step / np.sqrt((d0 * d0 + d1 * d1) + F32(1.0))
    n = H * W
    out = {"depth": np.zeros((B, n), F32), "voxel_id": np.full((B, n), -1, np.int32),
           "normal": np.zeros((B, n, 3), F32)}
    if vol["rgb"] is not None:
        out["rgb"] = np.zeros((B, n, 3), F32)
    if voxel_labels is not None:
        voxel_labels = np.asarray(voxel_labels, np.uint8)
        assert voxel_labels.shape == dims
        out["label"] = np.zeros((B, n), np.int32)
    evaluated = 0
    for b in range(B):
        P = poses[b]
        with np.errstate(all="ignore"):
            z_in = np.full(n, near, F32)
            z_out = np.full(n, far, F32)
            ok = np.ones(n, bool)
            q0, qd = [], []
            for a in range(3):
                w = (P[a, 0] * d0 + P[a, 1] * d1) + P[a, 2]
                q0a = np.full(n, (P[a, 3] - o[a]) / h[a], F32)
                qda = w / h[a]
                top = F32(dims[a] - 1)
                ok &= np.isfinite(q0a) & np.isfinite(qda)
                flat = qda == 0
                ok &= ~flat | ((q0a >= 0) & (q0a <= top))
                z1, z2 = (F32(0.0) - q0a) / qda, (top - q0a) / qda
                lo, hi = np.where(z1 < z2, z1, z2), np.where(z1 < z2, z2, z1)
                z_in = np.where(~flat & (lo > z_in), lo, z_in)
                z_out = np.where(~flat & (hi < z_out), hi, z_out)
                q0.append(q0a)
                qd.append(qda)
            ok &= (z_in <= z_out) & np.isfinite(z_in) & np.isfinite(z_out)
            ok &= (dz_all > 0) & np.isfinite(dz_all)
        ray = np.nonzero(ok)[0]            # rays still marching
        zh = np.zeros(n, F32)
        found = np.zeros(n, bool)
        k = 0
        while ray.size and k + 1 < MAXK:
            zi, dz = z_in[ray], dz_all[ray]
            zk, zk1 = zi + F32(k) * dz, zi + F32(k + 1) * dz
            go = zk1 <= z_out[ray]
            ray, zk, zk1, dz = ray[go], zk[go], zk1[go], dz[go]
            if not ray.size:
                break
            sub = [[q[ray] for q in q0], [q[ray] for q in qd]]
            c0, c1 = _Cells(dims, *sub, zk), _Cells(dims, *sub, zk1)
            ev = (c0.marked(marks) | c1.marked(marks)) if skip else np.ones(ray.size, bool)
            if ev.any():
                e = np.nonzero(ev)[0]
                sub = [[q[ray[e]] for q in q0], [q[ray[e]] for q in qd]]
                f0, v0 = _Cells(dims, *sub, zk[e]).sample(vol, min_weight)
                f1, v1 = _Cells(dims, *sub, zk1[e]).sample(vol, min_weight)
                evaluated += e.size
                hit = v0 & v1 & (f0 > 0) & (f1 <= 0)
                eh = e[hit]
                with np.errstate(all="ignore"):
                    z = zk[eh] + dz[eh] * (f0[hit] / (f0[hit] - f1[hit]))
                z = np.where(z < zk[eh], zk[eh], np.where(z > zk1[eh], zk1[eh], z))
                # a crossing whose own cell has an unobserved corner is no hit
                at = _Cells(dims, [q[ray[eh]] for q in q0], [q[ray[eh]] for q in qd], z)
                good = (at.corners(vol["weight"]) >= min_weight).all(0)
                eh, z = eh[good], z[good]
                zh[ray[eh]] = z
                found[ray[eh]] = True
                keep = np.ones(ray.size, bool)
                keep[eh] = False
                ray = ray[keep]
            k += 1
        r = np.nonzero(found)[0]
        cells = _Cells(dims, [q[r] for q in q0], [q[r] for q in qd], zh[r])
        idx = [np.clip(np.rint(cells.g[a]), F32(0), F32(dims[a] - 1)).astype(np.int64)
               for a in range(3)]
        vid = (idx[0] * dims[1] + idx[1]) * dims[2] + idx[2]
        out["depth"][b, r] = zh[r]
        out["voxel_id"][b, r] = vid.astype(np.int32)
        v = cells.corners(vol["tsdf"])
        c00, c01, c10, c11, c0, c1, f = cells.parts(v)
        G = [c1 - c0, _lerp(c01 - c00, c11 - c10, f[0]),
             _lerp(_lerp(v[1] - v[0], v[3] - v[2], f[1]), _lerp(v[5] - v[4], v[7] - v[6], f[1]),
                   f[0])]
        with np.errstate(all="ignore"):
            G = [G[a] / h[a] for a in range(3)]
            ln = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            good = (ln > 0) & np.isfinite(ln)
            nrm = np.stack([np.where(good, G[a] / ln, F32(0.0)) for a in range(3)], -1)
        out["normal"][b, r] = nrm
        if "rgb" in out:
            out["rgb"][b, r] = cells.trilerp(cells.corners(vol["rgb"]))
        if "label" in out:
            out["label"][b, r] = voxel_labels.reshape(-1)[vid].astype(np.int32)
    if stats is not None:
        stats["evaluated"] = stats.get("evaluated", 0) + evaluated
    out = {k2: v2.reshape((B, H, W) + v2.shape[2:]) for k2, v2 in out.items()}
    return out


def hit_cells(vol, poses, intrinsics, H, W, depth):
    """The cell [B,H,W,3] (int64) that holds each hit of a ``raycast`` depth map,
    by the contract's own arithmetic (rows of missed pixels are meaningless)."""
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    dims = vol["tsdf"].shape
    o, h = np.asarray(vol["origin"], F32), np.asarray(vol["spacing"], F32)
    ys, xs = np.mgrid[0:H, 0:W]
    d0 = ((xs.astype(F32) + F32(0.5)) - cx) / fx
    d1 = ((ys.astype(F32) + F32(0.5)) - cy) / fy
    out = np.zeros(depth.shape + (3,), np.int64)
    for b, P in enumerate(poses):
        q0 = [np.full((H, W), (P[a, 3] - o[a]) / h[a], F32) for a in range(3)]
        qd = [((P[a, 0] * d0 + P[a, 1] * d1) + P[a, 2]) / h[a] for a in range(3)]
        out[b] = np.stack(_Cells(dims, q0, qd, depth[b]).c, -1)
    return out
