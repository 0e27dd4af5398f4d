"""numpy restatement of the table-smoothing contracts of include/ucsa_hip.h
(``ucsa_voxel_table_smooth``, ``ucsa_label_table_smooth``) and of
``ops.mesh_adjacency``, written from the header comment: the yardstick the GPU
outputs are compared with, bit for bit (test infrastructure).

The lattice form is integer numpy over shifted slices, one add per offset; the
mesh form is ``np.add.at`` over the directed edge list; the adjacency comes from
a Python set of edges."""
import numpy as np

F32 = np.float32
SAT = {np.dtype(np.uint32): (1 << 32) - 1, np.dtype(np.uint16): 65535}


def offsets(neighbourhood):
    """the (dx, dy, dz) of N(v), the centre left out"""
    if neighbourhood not in (6, 26):
        raise ValueError("neighbourhood is 6 or 26")
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                taps = abs(dx) + abs(dy) + abs(dz)
                if taps and (neighbourhood == 26 or taps == 1):
                    out.append((dx, dy, dz))
    return out


def _shifted(n, d):
    """slices (destination, source) of an axis of length n so that source =
    destination + d stays inside"""
    return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))


def smooth_voxel_table(table, weight, neighbourhood=26, iterations=1, centre=1, min_weight=1.0):
    """table [C+1,nx,ny,nz] uint32 or uint16, weight [nx,ny,nz] fp32 -> a new
    table; the input is left alone."""
    table = np.asarray(table)
    sat = SAT[table.dtype]
    if not (isinstance(centre, (int, np.integer)) and 1 <= centre <= 255):
        raise ValueError("centre is an integer in 1..255")
    if iterations < 1:
        raise ValueError("iterations >= 1")
    obs = np.asarray(weight, F32) >= F32(min_weight)
    nx, ny, nz = obs.shape
    assert table.shape[1:] == obs.shape
    shifts = [tuple(_shifted(n, d) for n, d in zip((nx, ny, nz), o))
              for o in offsets(neighbourhood)]
    cur = table
    for _ in range(iterations):
        out = np.empty_like(cur)
        for p in range(cur.shape[0]):                           # a plane at a time: it stays in cache
            gated = np.where(obs, cur[p], 0).astype(np.uint64)  # what a voxel donates
            acc = cur[p].astype(np.uint64) * np.uint64(centre)
            for (ax, bx), (ay, by), (az, bz) in shifts:
                acc[ax, ay, az] += gated[bx, by, bz]
            pooled = np.minimum(acc, np.uint64(sat)).astype(table.dtype)
            out[p] = np.where(obs, pooled, cur[p])
        cur = out
    return cur


def mesh_adjacency(faces, n_vertices):
    """faces [F,3] -> offsets int32 [V+1], neighbours int32 [E]: every undirected
    edge once per direction, no self edges, no duplicates, ascending per vertex"""
    edges = set()
    for f in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                edges.add((a, b))
                edges.add((b, a))
    edges = sorted(edges)
    off = np.zeros(n_vertices + 1, np.int64)
    for a, _ in edges:
        assert 0 <= a < n_vertices
        off[a + 1] += 1
    return np.cumsum(off).astype(np.int32), np.array([b for _, b in edges], np.int32)


def smooth_label_table(votes, adjacency, iterations=1, centre=1):
    """votes [V,C+1] uint64 -> a new table, sums modulo 2^64"""
    off, nbr = adjacency
    votes = np.asarray(votes, np.uint64)
    src = np.repeat(np.arange(votes.shape[0]), np.diff(off.astype(np.int64)))
    cur = votes
    with np.errstate(over="ignore"):
        for _ in range(iterations):
            out = cur * np.uint64(centre)
            np.add.at(out, src, cur[nbr.astype(np.int64)])
            cur = out
    return cur
