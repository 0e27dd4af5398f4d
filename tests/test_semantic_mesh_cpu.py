"""CPU-only checks of the mesh export's conventions: the marching-cubes tables
from first principles, the numpy marching cubes that the GPU kernels are held
to (tests/mc_numpy.py), the PLY reader / writer, and the frame maps."""
import os
import re
from collections import Counter

import numpy as np
import pytest

from tests.mc_numpy import marching_cubes
from ucsa_neural_rendering_amd.utils import mc_tables as T
from ucsa_neural_rendering_amd.utils.ply import read_ply, write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _on_common_face(e1, e2):
    pts = [T.CORNERS[c] for c in set(T.EDGE_CORNERS[e1]) | set(T.EDGE_CORNERS[e2])]
    return any(len({p[a] for p in pts}) == 1 for a in range(3))


def test_tables_from_first_principles():
    assert len(T.TRI_TABLE) == 256
    for case, row in enumerate(T.TRI_TABLE):
        assert len(row) % 3 == 0 and len(row) <= 15
        out = [(case >> c) & 1 for c in range(8)]
        straddle = {e for e, (a, b) in enumerate(T.EDGE_CORNERS) if out[a] != out[b]}
        # only straddling edges, and every one of them
        assert set(row) == straddle, case
        # a triangle edge through the cube's interior is shared by exactly two
        # of the case's triangles; one on a cube face by one or two
        pairs = Counter()
        for t in range(0, len(row), 3):
            a, b, c = row[t:t + 3]
            assert len({a, b, c}) == 3, case
            for u, v in ((a, b), (b, c), (c, a)):
                pairs[frozenset((u, v))] += 1
        for pair, n in pairs.items():
            u, v = tuple(pair)
            if _on_common_face(u, v):
                assert n in (1, 2), (case, u, v, n)
            else:
                assert n == 2, (case, u, v, n)
    # the owner table names each edge's lower end and axis
    for e, (a, b) in enumerate(T.EDGE_CORNERS):
        lo = min(T.CORNERS[a], T.CORNERS[b])
        axis = [i for i in range(3) if T.CORNERS[a][i] != T.CORNERS[b][i]]
        assert T.EDGE_OWNER[e] == (*lo, axis[0])


def test_hip_table_is_the_python_table():
    src = open(os.path.join(ROOT, "ucsa_neural_rendering_amd", "csrc",
                            "marching_cubes.hip")).read()
    body = src.split("kTri[256][16] = {", 1)[1].split("};", 1)[0]
    rows = re.findall(r"\{([-0-9,\s]+)\}", body)
    assert len(rows) == 256
    for case, r in enumerate(rows):
        vals = [int(x) for x in r.split(",")]
        assert len(vals) == 16
        n = vals.index(-1) if -1 in vals else 16
        assert tuple(vals[:n]) == T.TRI_TABLE[case]
        assert all(x == -1 for x in vals[n:])
    owner = re.search(r"kEdgeOwner\[12\] = \{([^}]*)\}", src).group(1)
    packed = []
    for lit in owner.split(","):                    # "offset | axis << 3"
        off, axis = re.fullmatch(r"\s*(\d+) \| (\d+) << 3\s*", lit).groups()
        packed.append(int(off) | int(axis) << 3)
    assert packed == [o[0] | o[1] << 1 | o[2] << 2 | o[3] << 3 for o in T.EDGE_OWNER]


def _lattice(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n, dtype=np.float32)
    h = np.float32((hi - lo) / (n - 1))
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return X, Y, Z, h


def _topology(verts, faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    und, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    directed = np.unique(e, axis=0).shape[0]
    return und.shape[0], cnt, directed


def _area_volume(verts, faces):
    a, b, c = (verts[faces[:, i]].astype(np.float64) for i in range(3))
    n = np.cross(b - a, c - a)
    return 0.5 * np.linalg.norm(n, axis=1).sum(), np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6


def test_numpy_mc_sphere_closed_outward_and_accurate():
    X, Y, Z, h = _lattice(64)
    R = 0.7
    f = (R - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, fa, nr = marching_cubes(f, 0.0, (-1, -1, -1), (h, h, h))
    assert v.dtype == np.float32 and fa.dtype == np.int32 and nr.dtype == np.float32
    E, cnt, directed = _topology(v, fa)
    assert (cnt == 2).all()                          # closed 2-manifold
    assert directed == 3 * fa.shape[0]              # consistently oriented
    assert v.shape[0] - E + fa.shape[0] == 2        # Euler characteristic
    area, vol = _area_volume(v, fa)
    assert abs(area / (4 * np.pi * R * R) - 1) < 0.01
    assert abs(vol / (4 / 3 * np.pi * R ** 3) - 1) < 0.01   # > 0: faces point out
    a, b, c = (v[fa[:, i]] for i in range(3))
    fn = np.cross(b - a, c - a)
    assert ((fn * (a + b + c)).sum(1) > 0).all()    # every face outward
    assert ((nr * v).sum(1) > 0).all()              # every vertex normal outward
    assert np.allclose(np.linalg.norm(nr, axis=1), 1, atol=1e-5)
    assert np.abs(np.linalg.norm(v, axis=1) - R).max() < 0.5 * h


def test_numpy_mc_torus_euler_zero():
    X, Y, Z, h = _lattice(64)
    Rr, r = 0.55, 0.2
    q = np.sqrt(X * X + Y * Y) - Rr
    f = (r - np.sqrt(q * q + Z * Z)).astype(np.float32)
    v, fa, _ = marching_cubes(f, 0.0, (-1, -1, -1), (h, h, h))
    E, cnt, directed = _topology(v, fa)
    assert (cnt == 2).all() and directed == 3 * fa.shape[0]
    assert v.shape[0] - E + fa.shape[0] == 0
    area, vol = _area_volume(v, fa)
    assert abs(area / (4 * np.pi ** 2 * Rr * r) - 1) < 0.01
    assert abs(vol / (2 * np.pi ** 2 * Rr * r * r) - 1) < 0.01


def test_numpy_mc_conventions_on_one_edge():
    # 2x2x2 lattice, only point (0,0,0) inside: case 254, one triangle over the
    # three edges of point 0 (edge ids 0, 1, 2 -> vertices 0, 1, 2)
    f = np.zeros((2, 2, 2), np.float32)
    f[0, 0, 0] = 2.0
    v, fa, nr = marching_cubes(f, 0.5, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0))
    assert v.shape == (3, 3) and fa.shape == (1, 3)
    t = np.float32((np.float32(0.5) - np.float32(2.0)) / (np.float32(0.0) - np.float32(2.0)))
    assert v[0, 0] == np.float32(1.0) + t * np.float32(0.5)
    assert v[1, 1] == np.float32(2.0) + t * np.float32(0.25)
    assert v[2, 2] == np.float32(3.0) + t * np.float32(2.0)
    n = np.cross(v[fa[0, 1]] - v[fa[0, 0]], v[fa[0, 2]] - v[fa[0, 0]])
    assert (n > 0).all()                            # away from the inside corner
    # equality counts as outside; no crossing -> empty
    v, fa, nr = marching_cubes(np.full((3, 4, 5), 0.5, np.float32), 0.5)
    assert v.shape == (0, 3) and fa.shape == (0, 3)


def test_ply_round_trip_and_header(tmp_path):
    rng = np.random.default_rng(0)
    V = 50
    verts = rng.normal(size=(V, 3)).astype(np.float32)
    normals = rng.normal(size=(V, 3)).astype(np.float32)
    rgb = rng.random((V, 3)).astype(np.float32)
    labels = rng.integers(0, 41, V)
    faces = rng.integers(0, V, (30, 3)).astype(np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, verts, faces, normals, rgb, labels)
    raw = open(p, "rb").read()
    header = raw[:raw.index(b"end_header\n") + len(b"end_header\n")].decode()
    assert header == (
        "ply\nformat binary_little_endian 1.0\nelement vertex 50\n"
        "property float x\nproperty float y\nproperty float z\n"
        "property float nx\nproperty float ny\nproperty float nz\n"
        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
        "property ushort label\nelement face 30\n"
        "property list uchar int vertex_indices\nend_header\n")
    assert len(raw) == len(header) + V * (24 + 3 + 2) + 30 * 13
    m = read_ply(p)
    assert np.array_equal(m["verts"], verts) and np.array_equal(m["normals"], normals)
    assert np.array_equal(m["faces"], faces) and np.array_equal(m["labels"], labels)
    assert np.array_equal(m["rgb"], np.round(rgb * 255).astype(np.uint8))
    # vertices only
    write_ply(p, verts)
    m = read_ply(p)
    assert np.array_equal(m["verts"], verts) and "faces" not in m and "labels" not in m


def test_read_scannet_style_labelled_mesh(tmp_path):
    # the layout of ScanNet's *_vh_clean_2.labels.ply, written independently
    V, F = 7, 4
    rng = np.random.default_rng(1)
    vd = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"),
                   ("green", "u1"), ("blue", "u1"), ("alpha", "u1"), ("label", "<u2")])
    vert = np.zeros(V, vd)
    for k in "xyz":
        vert[k] = rng.normal(size=V)
    for k in ("red", "green", "blue", "alpha"):
        vert[k] = rng.integers(0, 256, V)
    vert["label"] = [0, 1, 40, 5, 5, 39, 2]
    fd = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    face = np.zeros(F, fd)
    face["n"] = 3
    face["i"] = rng.integers(0, V, (F, 3))
    header = ("ply\nformat binary_little_endian 1.0\ncomment VCGLIB generated\n"
              f"element vertex {V}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              "property uchar alpha\nproperty ushort label\n"
              f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n")
    p = str(tmp_path / "scene0000_00_vh_clean_2.labels.ply")
    with open(p, "wb") as f:
        f.write(header.encode() + vert.tobytes() + face.tobytes())
    m = read_ply(p)
    assert np.array_equal(m["labels"], [0, 1, 40, 5, 5, 39, 2])
    assert np.array_equal(m["verts"][:, 1], vert["y"])
    assert np.array_equal(m["alpha"], vert["alpha"])
    assert np.array_equal(m["faces"], face["i"])


def test_frame_maps_invert_nerf_matrix_to_ngp():
    from ucsa_neural_rendering_amd.dataset.ngp_utils import nerf_matrix_to_ngp
    from ucsa_neural_rendering_amd.utils.semantic_mesh import (ngp_to_pose_frame,
                                                              pose_frame_to_ngp)
    pose = np.eye(4)
    pose[:3, 3] = [0.5, -1.25, 2.0]          # a camera centre, scene units
    ngp = nerf_matrix_to_ngp(pose)[:3, 3][None]
    back = ngp_to_pose_frame(ngp)
    assert np.array_equal(back[0], pose[:3, 3])
    assert np.allclose(ngp_to_pose_frame(ngp, 2.0)[0], pose[:3, 3] / 2.0)
    assert np.array_equal(pose_frame_to_ngp(back), ngp)


def test_synthetic_room_labelled_mesh_is_ground_truth_shaped():
    from ucsa_neural_rendering_amd.dataset.synthetic_scene import SyntheticRoom
    room = SyntheticRoom(0, n_classes=40)
    m = room.labelled_mesh(step=0.1)
    v, f = m["verts"], m["faces"]
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert f.min() >= 0 and f.max() < v.shape[0]
    assert m["labels"].min() >= 1 and m["labels"].max() <= 40
    assert np.array_equal(m["labels"][f[:, 0]], m["face_classes"] + 1)
    # face normals point into the empty space (but for triangles of the
    # grid that straddle a box's footprint, whose corners are all free)
    a, b, c = (v[f[:, i]] for i in range(3))
    n = np.cross(b - a, c - a)
    q = (a + b + c) / 3 + 1e-3 * n / np.linalg.norm(n, axis=1, keepdims=True)
    free = (np.abs(q) < 3).all(1)
    for bb in room.boxes.numpy():
        free &= ~((q > bb[0]) & (q < bb[1])).all(1)
    assert free.mean() > 0.99
    import torch
    d, _ = room.nearest_surface(torch.from_numpy(v))
    assert float(d.max()) < 1e-6
