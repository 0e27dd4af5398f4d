"""numpy restatement of the label-fusion contract of
``ucsa_label_fuse_accumulate`` / ``ucsa_label_fuse_resolve`` (include/ucsa_hip.h),
written from the header comment: the yardstick the GPU tables are compared
with, bit for bit (test infrastructure).  ``fuse_views`` is the whole scheme on
the CPU, with ``tests/raster_numpy.py`` as the projection."""
import numpy as np

from tests import raster_numpy as R

F32 = np.float32


def new_table(V, C):
    """votes [V, C+1] uint64, zeroed; column 0 stays unused"""
    return np.zeros((V, C + 1), np.uint64)


def accumulate(votes, vertex_id, pred, weight=None, mesh_depth=None, sensor_depth=None,
               depth_tol=None):
    """In place; returns ``votes``.  Arrays of any (equal) shape."""
    V, C = votes.shape[0], votes.shape[1] - 1
    vid = np.asarray(vertex_id, np.int32).reshape(-1).astype(np.int64)
    cls = np.asarray(pred, np.uint8).reshape(-1).astype(np.int64)
    ok = (vid >= 1) & (vid <= V) & (cls >= 1) & (cls <= C)
    add = np.ones(vid.size, np.uint64)
    if weight is not None:
        w = np.asarray(weight, np.int32).reshape(-1).astype(np.int64)
        ok &= (w >= 0) & (w <= 65535)
        add = np.where(ok, w, 0).astype(np.uint64)
    if (mesh_depth is None) != (sensor_depth is None):
        raise ValueError("mesh_depth and sensor_depth come as a pair")
    if mesh_depth is not None:
        m = np.asarray(mesh_depth, F32).reshape(-1)
        s = np.asarray(sensor_depth, F32).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok &= (s > 0) & (np.abs(m - s) <= F32(depth_tol))  # NaN compares false
    np.add.at(votes, (vid[ok] - 1, cls[ok]), add[ok])
    return votes


def resolve(votes, min_votes=1):
    """-> label [V] int32, total [V] uint64, winner [V] uint64"""
    s = votes[:, 1:]
    total = s.sum(1, dtype=np.uint64)
    winner = s.max(1) if s.shape[0] else np.zeros(0, np.uint64)
    first = s.argmax(1) + 1 if s.shape[0] else np.zeros(0, np.int64)  # first maximum
    label = np.where(total >= np.uint64(min_votes), first, 0).astype(np.int32)
    return label, total, winner.astype(np.uint64)


def vertex_ids(mesh, poses, intr, H, W, near):
    """The rasterizer's vote target per pixel: [B,H,W] int32 1-based vertex id
    (0 = nothing), and the z-depth."""
    V = mesh["verts"].shape[0]
    out = R.rasterize(mesh["verts"], mesh["faces"], poses, intr, H, W, near,
                      np.arange(1, V + 1, dtype=np.int32))
    return out["label"], out["depth"]


def fuse_views(mesh, poses, intr, H, W, near, label_maps, depth_maps=None, depth_tol=None,
               weights=None, num_classes=40, min_votes=1):
    """The scheme of utils/mesh_fusion.fuse_views on the CPU -> dict labels,
    total, winner, observed, votes."""
    V = mesh["verts"].shape[0]
    votes = new_table(V, num_classes)
    poses = np.asarray(poses, F32).reshape(-1, 4, 4)
    for b in range(poses.shape[0]):
        vid, z = vertex_ids(mesh, poses[b:b + 1], intr, H, W, near)
        accumulate(votes, vid[0], np.asarray(label_maps[b], np.uint8),
                   None if weights is None else weights[b],
                   None if depth_maps is None else z[0],
                   None if depth_maps is None else depth_maps[b], depth_tol)
    label, total, winner = resolve(votes, min_votes)
    return {"labels": label, "total": total, "winner": winner,
            "observed": int((label > 0).sum()), "votes": votes}
