"""Vectorised numpy marching cubes with the conventions of
``ucsa_mc_count`` / ``ucsa_mc_emit`` (include/ucsa_hip.h): the yardstick the
GPU kernels are compared with, bit for bit (test infrastructure)."""
import numpy as np

from ucsa_neural_rendering_amd.utils import mc_tables as T

_TRI = np.full((256, 16), -1, np.int64)
for _c, _row in enumerate(T.TRI_TABLE):
    _TRI[_c, :len(_row)] = _row
NTRI = (_TRI >= 0).sum(1) // 3
_OWNER = np.array(T.EDGE_OWNER, np.int64)


def _neg_gradient(f, spacing):
    """-grad f per lattice point [nx,ny,nz,3]: central differences inside,
    one-sided on the boundary, divided by (index distance * spacing) in fp32."""
    g = np.empty(f.shape + (3,), np.float32)
    for a in range(3):
        n = f.shape[a]
        hi = np.minimum(np.arange(n) + 1, n - 1)
        lo = np.maximum(np.arange(n) - 1, 0)
        d = np.take(f, hi, axis=a) - np.take(f, lo, axis=a)
        h = (hi - lo).astype(np.float32) * np.float32(spacing[a])
        shape = [1, 1, 1]
        shape[a] = n
        g[..., a] = -(d / h.reshape(shape))
    return g


def marching_cubes(field, iso, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """field [nx,ny,nz] float32 -> verts [V,3] f32, faces [F,3] int32,
    normals [V,3] f32."""
    f = np.ascontiguousarray(field, dtype=np.float32)
    nx, ny, nz = f.shape
    iso = np.float32(iso)
    origin = np.asarray(origin, np.float32)
    spacing = np.asarray(spacing, np.float32)
    inside = f > iso
    # crossing edges, [nx,ny,nz,3] in edge-id order (3*point + axis)
    cross = np.zeros(f.shape + (3,), bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    edge_ids = np.nonzero(flat)[0]
    vid = np.full(flat.shape[0], -1, np.int64)
    vid[edge_ids] = np.arange(edge_ids.shape[0])
    point, axis = edge_ids // 3, edge_ids % 3
    i, j, k = np.unravel_index(point, f.shape)
    ijk = np.stack([i, j, k], 1)
    step = np.eye(3, dtype=np.int64)[axis]
    ijk1 = ijk + step
    f0 = f[i, j, k]
    f1 = f[ijk1[:, 0], ijk1[:, 1], ijk1[:, 2]]
    t = (iso - f0) / (f1 - f0)
    verts = origin[None, :] + ijk.astype(np.float32) * spacing[None, :]
    rows = np.arange(edge_ids.shape[0])
    verts[rows, axis] = verts[rows, axis] + t * spacing[axis]
    g = _neg_gradient(f, spacing)
    n0 = g[i, j, k]
    n1 = g[ijk1[:, 0], ijk1[:, 1], ijk1[:, 2]]
    n = n0 + t[:, None] * (n1 - n0)
    ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    ok = ln > 0
    normals = np.zeros_like(n)
    normals[ok] = n[ok] / ln[ok, None]
    # cells: case bit c set when corner c is outside
    out = ~inside
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    for c, (di, dj, dk) in enumerate(T.CORNERS):
        case |= out[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << c
    ci, cj, ck = np.nonzero(NTRI[case] > 0)  # ascending cell index
    cc = case[ci, cj, ck]
    nt = NTRI[cc]
    cell = np.repeat(np.arange(cc.shape[0]), nt)
    slot = np.arange(cell.shape[0]) - np.repeat(np.cumsum(nt) - nt, nt)
    faces = np.empty((cell.shape[0], 3), np.int64)
    for m in range(3):
        e = _TRI[cc[cell], 3 * slot + m]
        o = _OWNER[e]
        pi = ci[cell] + o[:, 0]
        pj = cj[cell] + o[:, 1]
        pk = ck[cell] + o[:, 2]
        faces[:, m] = vid[3 * ((pi * ny + pj) * nz + pk) + o[:, 3]]
    assert (faces >= 0).all()
    return verts.astype(np.float32), faces.astype(np.int32), normals.astype(np.float32)
