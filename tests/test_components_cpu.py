"""CPU-only: the numpy restatement of the connected-component contracts
(tests/components_numpy.py) against an independent breadth-first flood fill on
small random lattices and graphs, and on hand-written cases."""
from collections import deque

import numpy as np
import pytest

from tests import components_numpy as CN


def flood_lattice(mask, connectivity):
    """component minima by breadth-first search, voxel by voxel"""
    m = np.asarray(mask) != 0
    nx, ny, nz = m.shape
    if connectivity == 6:
        offs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    else:
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
                if (a, b, c) != (0, 0, 0)]
    out = np.full(m.shape, -1, np.int32)
    for i, j, k in zip(*np.nonzero(m)):          # ascending linear index: the first is the minimum
        if out[i, j, k] >= 0:
            continue
        root = (i * ny + j) * nz + k
        out[i, j, k] = root
        queue = deque([(i, j, k)])
        while queue:
            x, y, z = queue.popleft()
            for a, b, c in offs:
                u, v, w = x + a, y + b, z + c
                if 0 <= u < nx and 0 <= v < ny and 0 <= w < nz and m[u, v, w] and out[u, v, w] < 0:
                    out[u, v, w] = root
                    queue.append((u, v, w))
    return out


def flood_graph(offsets, neighbours):
    V = len(offsets) - 1
    out = np.full(V, -1, np.int32)
    for s in range(V):
        if out[s] >= 0:
            continue
        out[s] = s
        queue = deque([s])
        while queue:
            v = queue.popleft()
            for n in neighbours[offsets[v]:offsets[v + 1]]:
                if out[n] < 0:
                    out[n] = s
                    queue.append(int(n))
    return out


def check_labelling(mask, lab):
    m = np.asarray(mask) != 0
    flat = lab.reshape(-1)
    assert lab.dtype == np.int32 and (lab[~m] == -1).all() and (lab[m] >= 0).all()
    # a label is an element of its own component, and the smallest one
    roots = np.unique(flat[flat >= 0])
    assert (flat[roots] == roots).all()
    assert (flat[flat >= 0] <= np.flatnonzero(flat >= 0)).all()
    sizes = CN.component_sizes(lab)
    assert sizes.dtype == np.int32 and sizes.shape == lab.shape
    assert (sizes[~m] == 0).all() and int(sizes.reshape(-1)[roots].sum()) == int(m.sum())


@pytest.mark.parametrize("connectivity", [6, 26])
def test_restatement_matches_a_flood_fill_on_random_lattices(connectivity):
    g = np.random.default_rng(connectivity)
    for dims in ((7, 6, 9), (1, 1, 12), (3, 11, 2), (2, 2, 2)):
        for density in (0.1, 0.32, 0.7):
            m = g.random(dims) < density
            lab = CN.voxel_components(m.astype(np.uint8) * 3, connectivity)
            assert lab.tobytes() == flood_lattice(m, connectivity).tobytes(), (dims, density)
            check_labelling(m, lab)


def test_restatement_matches_a_flood_fill_on_random_graphs():
    g = np.random.default_rng(5)
    for V, F in ((40, 25), (200, 90), (9, 0)):
        faces = g.integers(0, V, (F, 3))
        off, nbr = CN.mesh_adjacency(faces, V)
        lab = CN.graph_components(off, nbr)
        assert lab.dtype == np.int32 and lab.tobytes() == flood_graph(off, nbr).tobytes()
        sizes = CN.component_sizes(lab)
        assert sizes.sum() == sum(int(s) ** 2 for s in sizes[lab == np.arange(V)])


def test_hand_written_lattices():
    m = np.zeros((3, 3, 3), bool)
    m[0, 0, 0] = m[1, 1, 1] = True                 # touching only at a corner
    assert len(np.unique(CN.voxel_components(m, 6)[m])) == 2
    lab = CN.voxel_components(m, 26)
    assert lab[0, 0, 0] == 0 and lab[1, 1, 1] == 0
    i, j, k = np.indices((4, 5, 6))
    board = (i + j + k) % 2 == 0                    # a 3-D checkerboard
    lab = CN.voxel_components(board, 6)
    assert (lab[board] == np.flatnonzero(board.reshape(-1))).all()      # all singletons
    assert (CN.component_sizes(lab)[board] == 1).all()
    lab = CN.voxel_components(board, 26)
    assert (lab[board] == 0).all() and CN.component_sizes(lab)[0, 0, 0] == board.sum()
    empty = np.zeros((3, 4, 5), bool)
    assert (CN.voxel_components(empty, 26) == -1).all()
    assert (CN.component_sizes(CN.voxel_components(empty, 6)) == 0).all()
    full = np.ones((3, 4, 5), bool)
    for c in (6, 26):
        lab = CN.voxel_components(full, c)
        assert (lab == 0).all() and (CN.component_sizes(lab) == 60).all()
    with pytest.raises(ValueError):
        CN.voxel_components(full, 18)


def test_graph_with_isolated_vertices_and_sizes_with_negative_labels():
    faces = np.array([[0, 1, 2], [2, 3, 3], [6, 7, 8]])
    off, nbr = CN.mesh_adjacency(faces, 11)
    lab = CN.graph_components(off, nbr)
    assert lab.tolist() == [0, 0, 0, 0, 4, 5, 6, 6, 6, 9, 10]
    assert CN.component_sizes(lab).tolist() == [4, 4, 4, 4, 1, 1, 3, 3, 3, 1, 1]
    assert CN.component_sizes(np.array([-1, 2, 2, -1, 2, 0], np.int32)).tolist() == \
        [0, 3, 3, 0, 3, 1]
    assert CN.graph_components(np.zeros(1, np.int32), np.zeros(0, np.int32)).size == 0


def test_serpentine_is_one_long_component_and_the_restatement_is_quick():
    import time
    dims = (37, 20, 65)
    m = CN.serpentine(dims)
    t0 = time.perf_counter()
    labs = {c: CN.voxel_components(m, c) for c in (6, 26)}
    g = np.random.default_rng(0)
    rnd = CN.voxel_components(g.random(dims) < 0.32, 6)
    dt = (time.perf_counter() - t0) / 3
    print(f"restatement: {dt:.3f} s per 37 x 20 x 65 lattice")
    for lab in labs.values():
        assert (lab[m] == 0).all() and m[0, 0, 0]
    assert m.sum() > 10000 and (rnd >= 0).any()
    assert lab.tobytes() == flood_lattice(m, 26).tobytes()


def test_remove_small_components_and_filter_mesh_components():
    vol = {"tsdf": np.ones((6, 6, 12), np.float32), "weight": np.zeros((6, 6, 12), np.float32),
           "rgb": np.zeros((6, 6, 12, 3), np.float32)}
    vol["weight"][:] = 2.0
    vol["tsdf"][2, :, :] = 0.25                      # a wall: 72 voxels
    vol["tsdf"][5, 5, 10:12] = -0.5                  # a speck: 2 voxels
    vol["weight"][0, 0, 0] = np.nan
    vol["tsdf"][0, 0, 0] = 0.0                       # never observed: not in the band
    vol["rgb"][...] = 7.0
    before = {k: v.copy() for k, v in vol.items()}
    st = CN.remove_small_components(vol, 1)
    assert st == {"components": 2, "removed_components": 0, "removed_voxels": 0, "largest": 72}
    assert all(vol[k].tobytes() == before[k].tobytes() for k in vol)
    st = CN.remove_small_components(vol, 3, connectivity=6)
    assert st == {"components": 2, "removed_components": 1, "removed_voxels": 2, "largest": 72}
    assert (vol["tsdf"][5, 5, 10:12] == 1).all() and (vol["weight"][5, 5, 10:12] == 0).all()
    assert (vol["rgb"][5, 5, 10:12] == 0).all() and (vol["tsdf"][2] == 0.25).all()
    assert np.isnan(vol["weight"][0, 0, 0])
    # two triangles sharing an edge (4 vertices), a lone triangle, an unused vertex
    mesh = {"verts": np.arange(24, dtype=np.float32).reshape(8, 3),
            "faces": np.array([[4, 5, 6], [0, 1, 2], [1, 2, 3]], np.int32),
            "labels": np.arange(8, dtype=np.int32), "rgb": None}
    out, st = CN.filter_mesh_components(mesh, min_vertices=3)
    assert st == {"components": 3, "removed_components": 1, "removed_vertices": 1, "largest": 4}
    assert out["labels"].tolist() == [0, 1, 2, 3, 4, 5, 6] and out["rgb"] is None
    assert out["faces"].tolist() == [[4, 5, 6], [0, 1, 2], [1, 2, 3]]
    out, st = CN.filter_mesh_components(mesh, keep_largest=1)
    assert out["faces"].tolist() == [[0, 1, 2], [1, 2, 3]] and st["removed_vertices"] == 4
    assert out["vertex_index"].tolist() == [0, 1, 2, 3] and out["face_index"].tolist() == [1, 2]
    out, st = CN.filter_mesh_components(mesh, min_vertices=4, keep_largest=2)
    assert out["verts"].shape == (4, 3) and st["removed_components"] == 2
    # ties go to the smaller label
    tie = {"verts": np.zeros((6, 3), np.float32),
           "faces": np.array([[3, 4, 5], [0, 1, 2]], np.int32)}
    out, st = CN.filter_mesh_components(tie, keep_largest=1)
    assert out["vertex_index"].tolist() == [0, 1, 2] and out["faces"].tolist() == [[0, 1, 2]]
