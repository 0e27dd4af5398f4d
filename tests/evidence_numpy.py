"""numpy restatement of the soft label fusion contracts of include/ucsa_hip.h:
``ops.log_evidence`` in float64 and ``ucsa_tsdf_evidence``,
``ucsa_voxel_evidence_resolve`` and ``ucsa_label_fuse_evidence`` in integers,
written from the header comment: the yardstick the GPU outputs are compared
with, bit for bit (test infrastructure).

Which voxels a view reaches is decided by ``tests/voxel_map_numpy.vote`` itself
(one class, every pixel voting: its plane 1 is the band of the view), so the
projection and the skip tests exist once; only the pixel that a voxel of the
band reads is worked out here, with the same two lines of fp32."""
import numpy as np

from tests import tsdf_numpy as TN
from tests import voxel_map_numpy as VN

F32 = np.float32
SAT = (1 << 32) - 1


def log_evidence(x, from_logits=False, floor_nats=8.0):
    """x [B,C,H,W] -> uint8 [B,H,W,C]: e = 255 - rint(255 * min(-ln p, L) / L) in
    float64 (the values of x taken as they are, in whatever precision)."""
    x = np.asarray(x).astype(np.float64)
    L = float(floor_nats)
    with np.errstate(all="ignore"):
        if from_logits:
            m = x.max(1, keepdims=True)
            nl = -(x - m - np.log(np.exp(x - m).sum(1, keepdims=True)))
        else:
            nl = -np.log(x)
    nl = np.clip(np.nan_to_num(nl, nan=L, posinf=L, neginf=0.0), 0.0, L)
    e = 255.0 - np.rint(255.0 * nl / L)
    return np.ascontiguousarray(e.astype(np.uint8).transpose(0, 2, 3, 1))


def new_evidence(dims, n_classes):
    assert 1 <= n_classes <= 255
    return np.zeros((n_classes + 1,) + tuple(int(d) for d in dims), np.uint32)


def view_band(vol, depth, pose, intrinsics, trunc, depth_min=1e-6, depth_max=3.0e38):
    """-> band [nx,ny,nz] bool (the voxels that the view reaches under
    ucsa_tsdf_vote's rule), and the pixel (v, u) each voxel projects to
    (int64, meaningful inside the band)."""
    depth = np.asarray(depth, F32)
    H, W = depth.shape
    dims = vol["tsdf"].shape
    one = VN.vote(VN.new_votes(dims, 1), vol, depth[None], np.ones((1, H, W), np.uint8),
                  np.asarray(pose, F32).reshape(1, 4, 4), intrinsics, trunc, depth_min,
                  depth_max)
    band = one[1] > 0
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    P = np.asarray(pose, F32).reshape(4, 4)
    px, py, pz = TN.voxel_centres(vol)
    d0, d1, d2 = px - P[0, 3], py - P[1, 3], pz - P[2, 3]
    c = [np.broadcast_to((d0 * P[0, r] + d1 * P[1, r]) + d2 * P[2, r], dims) for r in range(3)]
    with np.errstate(all="ignore"):
        u = np.floor((fx * c[0]) / c[2] + cx)
        v = np.floor((fy * c[1]) / c[2] + cy)
    ui = np.where(band, u, 0).astype(np.int64)
    vi = np.where(band, v, 0).astype(np.int64)
    assert (ui >= 0).all() and (ui < W).all() and (vi >= 0).all() and (vi < H).all()
    return band, vi, ui


def accumulate(ev, vol, depth, scores, poses, intrinsics, trunc, depth_min=1e-6,
               depth_max=3.0e38, reached=None):
    """In place; returns ``ev``.  scores [B,H,W,C] uint8.  ``reached``: a bool
    array [nx,ny,nz] that collects the voxels with an in-band view."""
    depth = np.asarray(depth, F32)
    scores = np.asarray(scores, np.uint8)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    B, H, W = depth.shape
    Cn = ev.shape[0] - 1
    assert poses.shape[0] == B and scores.shape == (B, H, W, Cn)
    for b in range(B):
        band, vi, ui = view_band(vol, depth[b], poses[b], intrinsics, trunc, depth_min,
                                 depth_max)
        if reached is not None:
            reached |= band
        i, j, k = np.nonzero(band)
        rows = scores[b][vi[i, j, k], ui[i, j, k]]          # [n, C]
        keep = rows.any(1)                                   # an all-zero row abstains
        i, j, k, rows = i[keep], j[keep], k[keep], rows[keep]
        cur = ev[:, i, j, k].astype(np.uint64)               # voxels are distinct
        cur[1:] += rows.T.astype(np.uint64)
        cur[0] += np.uint64(1)
        ev[:, i, j, k] = np.minimum(cur, np.uint64(SAT)).astype(np.uint32)
    return ev


def resolve(ev, min_views=1, min_margin=0):
    """-> label [nx,ny,nz] uint8, views, best, margin uint32"""
    s = ev[1:]
    views = ev[0].copy()
    arg = np.argmax(s, 0)                                    # the first maximum: the lowest class
    best = s.max(0)
    if s.shape[0] > 1:
        rest = s.astype(np.int64)
        np.put_along_axis(rest, arg[None], -1, 0)
        second = rest.max(0).astype(np.uint32)
    else:
        second = np.zeros_like(best)
    margin = (best - second).astype(np.uint32)
    ok = (views >= np.uint32(min_views)) & (margin >= np.uint32(min_margin))
    label = np.where(ok, arg + 1, 0).astype(np.uint8)
    return label, views, best, margin


def fuse(votes, vertex_id, scores, mesh_depth=None, sensor_depth=None, depth_tol=None):
    """ucsa_label_fuse_evidence on the table of tests/fusion_numpy.new_table, in
    place; returns ``votes``.  scores: vertex_id's shape + (C,)."""
    V, C = votes.shape[0], votes.shape[1] - 1
    vid = np.asarray(vertex_id, np.int32).reshape(-1).astype(np.int64)
    rows = np.asarray(scores, np.uint8).reshape(-1, C)
    assert rows.shape[0] == vid.size
    ok = (vid >= 1) & (vid <= V)
    if (mesh_depth is None) != (sensor_depth is None):
        raise ValueError("mesh_depth and sensor_depth come as a pair")
    if mesh_depth is not None:
        m = np.asarray(mesh_depth, F32).reshape(-1)
        s = np.asarray(sensor_depth, F32).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok &= (s > 0) & (np.abs(m - s) <= F32(depth_tol))
    np.add.at(votes[:, 1:], vid[ok] - 1, rows[ok].astype(np.uint64))
    return votes
