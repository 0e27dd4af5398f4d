"""numpy float32 restatement of the depth front end's contracts in
include/ucsa_hip.h (``ucsa_depth_filter``, ``ucsa_depth_normals``,
``ucsa_depth_frontend``), written from the header comments as plain loops over
the pixels: the yardstick the GPU outputs are compared with, bit for bit (test
infrastructure).  It knows nothing of tiles, halos or LDS.  ``filter_vec`` and
``normals_vec`` are the same contracts with the pixel loops turned into array
operations (the window offsets stay a loop, in the contract's order), for the
frames too large for the loops; tests/test_depth_frontend_cpu.py holds them to
the loops' bytes."""
import numpy as np

F32 = np.float32
Q = 256
MEASURED, NORMAL, EDGE, GRAZING = 1, 2, 4, 8


def bilateral_tables(radius, sigma_space):
    """the tables of ops.depth.bilateral_tables, restated"""
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = k[:, None] ** 2 + k[None, :] ** 2
    q = np.arange(Q, dtype=np.float64)
    return {"radius": int(radius),
            "w_space": np.exp(-d2 / (2.0 * float(sigma_space) ** 2)).astype(F32).reshape(-1),
            "w_range": np.exp(-0.5 * ((q + 0.5) * 3.0 / Q) ** 2).astype(F32)}


def _measured(z, dmin, dmax):
    return bool(np.isfinite(z) and z >= dmin and z <= dmax)


def filter(depth, tables, sigma_depth, sigma_z2=0.0, depth_min=1e-6, depth_max=3.0e38):
    """ucsa_depth_filter -> filtered [B,H,W] float32"""
    depth = np.asarray(depth, F32)
    B, H, W = depth.shape
    r = int(tables["radius"])
    ws, wr = np.asarray(tables["w_space"], F32), np.asarray(tables["w_range"], F32)
    sd, s2, dmin, dmax = F32(sigma_depth), F32(sigma_z2), F32(depth_min), F32(depth_max)
    out = np.zeros((B, H, W), F32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(H):
                for j in range(W):
                    z = depth[b, i, j]
                    if not _measured(z, dmin, dmax):
                        continue
                    sigma = sd + s2 * (z * z)
                    scale = F32(Q) / (F32(3.0) * sigma)
                    num, den = F32(0.0), F32(0.0)
                    for dy in range(-r, r + 1):
                        for dx in range(-r, r + 1):
                            ii, jj = i + dy, j + dx
                            if not (0 <= ii < H and 0 <= jj < W):
                                continue
                            zn = depth[b, ii, jj]
                            if not _measured(zn, dmin, dmax):
                                continue
                            d = zn - z
                            t = np.abs(d) * scale
                            if not t < F32(Q):
                                continue
                            w = ws[(dy + r) * (2 * r + 1) + (dx + r)] * wr[int(t)]
                            num = num + w * d
                            den = den + w
                    out[b, i, j] = z + num / den
    return out


def _point(i, j, z, K):
    fx, fy, cx, cy = K
    return np.array([(((F32(j) + F32(0.5)) - cx) / fx) * z, (((F32(i) + F32(0.5)) - cy) / fy) * z,
                     z], F32)


def normals(depth, intrinsics, max_jump, max_jump_z2=0.0, min_cos=0.0, depth_min=1e-6,
            depth_max=3.0e38):
    """ucsa_depth_normals -> points [B,H,W,3] f32, normals [B,H,W,3] f32, mask [B,H,W] u8"""
    depth = np.asarray(depth, F32)
    B, H, W = depth.shape
    K = tuple(F32(v) for v in intrinsics)
    mj, mj2, mc = F32(max_jump), F32(max_jump_z2), F32(min_cos)
    dmin, dmax = F32(depth_min), F32(depth_max)
    points = np.zeros((B, H, W, 3), F32)
    nrm = np.zeros((B, H, W, 3), F32)
    mask = np.zeros((B, H, W), np.uint8)
    with np.errstate(all="ignore"):
        for b in range(B):
            for i in range(H):
                for j in range(W):
                    z = depth[b, i, j]
                    if not _measured(z, dmin, dmax):
                        continue
                    m = MEASURED
                    p = _point(i, j, z, K)
                    points[b, i, j] = p
                    thr = mj + mj2 * (z * z)

                    def look(ii, jj):
                        """(measured, usable, depth) of a neighbour"""
                        if not (0 <= ii < H and 0 <= jj < W):
                            return False, False, F32(0)
                        zn = depth[b, ii, jj]
                        meas = _measured(zn, dmin, dmax)
                        return meas, bool(meas and np.abs(zn - z) <= thr), zn

                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            meas, use, _ = look(i + dy, j + dx)
                            if (dy or dx) and meas and not use:
                                m |= EDGE

                    def diff(minus, plus):
                        _, um, zm = look(*minus)
                        _, up, zp = look(*plus)
                        if not (um or up):
                            return None
                        lo = _point(minus[0], minus[1], zm, K) if um else p
                        hi = _point(plus[0], plus[1], zp, K) if up else p
                        return hi - lo

                    du = diff((i, j - 1), (i, j + 1))
                    dv = diff((i - 1, j), (i + 1, j))
                    if du is not None and dv is not None:
                        c = np.array([dv[1] * du[2] - dv[2] * du[1],
                                      dv[2] * du[0] - dv[0] * du[2],
                                      dv[0] * du[1] - dv[1] * du[0]], F32)
                        nn = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
                        if nn > 0 and np.isfinite(nn):
                            n = c / np.sqrt(nn)
                            dot = (n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]
                            if dot > 0:
                                n, dot = -n, -dot
                            cosv = (-dot) / np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2])
                            m |= NORMAL
                            if cosv < mc:
                                m |= GRAZING
                            nrm[b, i, j] = n
                    mask[b, i, j] = m
    return points, nrm, mask


def frontend(depth, tables, intrinsics, sigma_depth, max_jump, sigma_z2=0.0, max_jump_z2=0.0,
             min_cos=0.0, reject=EDGE | GRAZING, depth_min=1e-6, depth_max=3.0e38,
             filter_fn=None, normals_fn=None):
    """ucsa_depth_frontend: the two above, and clean -> dict as ops.depth.depth_frontend"""
    f = (filter_fn or filter)(depth, tables, sigma_depth, sigma_z2, depth_min, depth_max)
    points, nrm, mask = (normals_fn or normals)(f, intrinsics, max_jump, max_jump_z2, min_cos,
                                                depth_min, depth_max)
    clean = np.where((mask & np.uint8(reject)) != 0, F32(0.0), f).astype(F32)
    return {"depth": f, "clean": clean, "points": points, "normals": nrm, "mask": mask}


# ---------------------------------------------------------------------------
# the same contracts over whole arrays
# ---------------------------------------------------------------------------
def _shift(a, dy, dx, fill):
    """out[..., i, j] = a[..., i+dy, j+dx], ``fill`` outside the image"""
    out = np.full_like(a, fill)
    H, W = a.shape[-2:]
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def _measured_vec(z, dmin, dmax):
    return np.isfinite(z) & (z >= dmin) & (z <= dmax)


def filter_vec(depth, tables, sigma_depth, sigma_z2=0.0, depth_min=1e-6, depth_max=3.0e38):
    depth = np.asarray(depth, F32)
    r = int(tables["radius"])
    ws, wr = np.asarray(tables["w_space"], F32), np.asarray(tables["w_range"], F32)
    sd, s2, dmin, dmax = F32(sigma_depth), F32(sigma_z2), F32(depth_min), F32(depth_max)
    with np.errstate(all="ignore"):
        z = depth
        ok = _measured_vec(z, dmin, dmax)
        sigma = sd + s2 * (z * z)
        scale = F32(Q) / (F32(3.0) * sigma)
        num, den = np.zeros_like(z), np.zeros_like(z)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                zn = _shift(z, dy, dx, F32(np.nan))
                d = zn - z
                t = np.abs(d) * scale
                take = ok & _measured_vec(zn, dmin, dmax) & (t < F32(Q))
                q = np.where(take, t, F32(0)).astype(np.int64)
                w = ws[(dy + r) * (2 * r + 1) + (dx + r)] * wr[q]
                num = np.where(take, num + w * d, num)
                den = np.where(take, den + w, den)
        return np.where(ok, z + num / den, F32(0.0)).astype(F32)


def normals_vec(depth, intrinsics, max_jump, max_jump_z2=0.0, min_cos=0.0, depth_min=1e-6,
                depth_max=3.0e38):
    depth = np.asarray(depth, F32)
    B, H, W = depth.shape
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    mj, mj2, mc = F32(max_jump), F32(max_jump_z2), F32(min_cos)
    dmin, dmax = F32(depth_min), F32(depth_max)
    with np.errstate(all="ignore"):
        z = depth
        ok = _measured_vec(z, dmin, dmax)
        ax = (((np.arange(W, dtype=F32) + F32(0.5)) - cx) / fx)[None, None, :]
        ay = (((np.arange(H, dtype=F32) + F32(0.5)) - cy) / fy)[None, :, None]
        P = np.stack([ax * z, ay * z, z], -1).astype(F32)
        thr = mj + mj2 * (z * z)
        edge = np.zeros(z.shape, bool)
        use = {}
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                zn = _shift(z, dy, dx, F32(np.nan))
                meas = _measured_vec(zn, dmin, dmax)
                use[dy, dx] = meas & (np.abs(zn - z) <= thr)
                if dy or dx:
                    edge |= meas & ~use[dy, dx]

        def diff(minus, plus):
            um, up = use[minus][..., None], use[plus][..., None]
            Pm = np.moveaxis(_shift(np.moveaxis(P, -1, 0), minus[0], minus[1], F32(0)), 0, -1)
            Pp = np.moveaxis(_shift(np.moveaxis(P, -1, 0), plus[0], plus[1], F32(0)), 0, -1)
            return np.where(up, Pp, P) - np.where(um, Pm, P), (um | up)[..., 0]

        du, hu = diff((0, -1), (0, 1))
        dv, hv = diff((-1, 0), (1, 0))
        c = np.stack([dv[..., 1] * du[..., 2] - dv[..., 2] * du[..., 1],
                      dv[..., 2] * du[..., 0] - dv[..., 0] * du[..., 2],
                      dv[..., 0] * du[..., 1] - dv[..., 1] * du[..., 0]], -1)
        nn = (c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]
        has = ok & hu & hv & (nn > 0) & np.isfinite(nn)
        n = c / np.sqrt(nn)[..., None]
        dot = (n[..., 0] * P[..., 0] + n[..., 1] * P[..., 1]) + n[..., 2] * P[..., 2]
        flip = dot > 0
        n = np.where(flip[..., None], -n, n)
        dot = np.where(flip, -dot, dot)
        cosv = (-dot) / np.sqrt((P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1])
                                + P[..., 2] * P[..., 2])
        mask = (ok * MEASURED + has * NORMAL + (ok & edge) * EDGE
                + (has & (cosv < mc)) * GRAZING).astype(np.uint8)
        points = np.where(ok[..., None], P, F32(0.0)).astype(F32)
        nrm = np.where(has[..., None], n, F32(0.0)).astype(F32)
    return points, nrm, mask


def frontend_vec(*args, **kw):
    return frontend(*args, filter_fn=filter_vec, normals_fn=normals_vec, **kw)
