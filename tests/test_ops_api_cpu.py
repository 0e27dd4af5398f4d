"""The surface of ``ucsa_neural_rendering_amd.ops`` is frozen: every name that
was reachable as ``ops.NAME`` when it was one file is reachable from the package
with the same signature, docstring and value (tests/golden/ops_api.json, taken
with ``snapshot()`` below from the single-file module), and the ops that take
tensors turn CPU tensors away before they reach the library.  No GPU needed."""
import __future__

import hashlib
import inspect
import json
import os

import pytest
import torch

from ucsa_neural_rendering_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_api.json")
# private names that tests, tools and the renderer reach through ``ops``
PRIVATE = ("_lib", "_ptr", "_stream", "_scratch", "_bwd_ws")
# public names the package has and the single file had not
ADDED = {"volume_lattice"}


def _doc(obj):
    d = inspect.getdoc(obj)
    return None if d is None else hashlib.sha256(d.encode()).hexdigest()


def _func(f):
    return {"signature": str(inspect.signature(f)), "doc": _doc(f)}


def _public(mod):
    return {k: v for k, v in vars(mod).items()
            if not k.startswith("_") and not inspect.ismodule(v)
            and getattr(v, "__module__", None) != "typing"
            and not isinstance(v, __future__._Feature)}


def snapshot(mod):
    snap = {"functions": {}, "classes": {}, "constants": {}}
    for name, v in sorted(_public(mod).items()):
        if inspect.isclass(v):
            snap["classes"][name] = {
                "doc": _doc(v),
                "methods": {m: _func(f) for m, f in sorted(vars(v).items())
                            if inspect.isfunction(f)}}
        elif inspect.isfunction(v):
            snap["functions"][name] = _func(v)
        else:
            snap["constants"][name] = v
    return snap


def test_names_signatures_docstrings_and_constants_match_the_snapshot():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = snapshot(ops)
    for kind in ("functions", "classes", "constants"):
        assert set(got[kind]) - ADDED == set(want[kind]), kind
        for name in want[kind]:
            assert got[kind][name] == want[kind][name], (kind, name)
    assert len(want["functions"]) == 105 + 3      # the ops; lib, check, fvec
    assert set(want["classes"]) == {"Grid", "MarchSegments"}
    assert len(want["constants"]) == 9
    for name in PRIVATE:
        assert hasattr(ops, name), name


def test_private_state_is_shared_not_copied():
    assert ops._lib is _lib
    assert ops._bwd_ws is ops.backward._bwd_ws
    assert ops._march_ws is ops._args._march_ws
    assert ops._named_ws is ops._args._named_ws
    assert ops._scratch is ops._args._scratch
    for d in (ops._bwd_ws, ops._march_ws, ops._named_ws):
        assert isinstance(d, dict)


# ---------------------------------------------------------------------------
# CPU tensors of valid shapes: UcsaError before the library is reached
# ---------------------------------------------------------------------------
class ReachedLibrary(Exception):
    pass


def _cpu_calls():
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    volume = {"tsdf": torch.ones(5, 4, 3), "weight": torch.zeros(5, 4, 3), "rgb": None,
              "origin": (0.0, 0.0, 0.0), "spacing": (0.1, 0.1, 0.1)}
    depth = torch.ones(2, 6, 8)
    poses = torch.eye(4).repeat(2, 1, 1)
    K = (8.0, 8.0, 4.0, 3.0)
    pred = torch.ones(2, 6, 8, dtype=u8)
    scores = torch.ones(2, 6, 8, 3, dtype=u8)
    votes16 = torch.zeros(4, 5, 4, 3, dtype=torch.uint16)
    evidence32 = torch.zeros(4, 5, 4, 3, dtype=torch.uint32)
    verts = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=f32)
    faces = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=i32)
    table = torch.zeros(4, 4, dtype=torch.int64)
    vertex_id = torch.ones(2, 6, 8, dtype=i32)
    adjacency = (torch.tensor([0, 2, 4, 6, 8], dtype=i32),
                 torch.tensor([1, 2, 0, 3, 0, 3, 1, 2], dtype=i32))
    grid = {"sorted_points": torch.zeros(4, 4), "offsets": torch.zeros(2, dtype=i32),
            "origin": (0.0, 0.0, 0.0), "cell": 1.0, "dims": (1, 1, 1), "n": 4}
    return {
        "integrate_tsdf": lambda: ops.integrate_tsdf(volume, depth, poses, K, 0.3),
        "vote_voxel_labels": lambda: ops.vote_voxel_labels(votes16, volume, depth, pred, poses,
                                                           K, 0.3),
        "accumulate_voxel_evidence": lambda: ops.accumulate_voxel_evidence(
            evidence32, volume, depth, scores, poses, K, 0.3),
        "raycast_tsdf": lambda: ops.raycast_tsdf(volume, poses, K, 6, 8, 0.1, 4.0, trunc=0.3),
        "rasterize_mesh": lambda: ops.rasterize_mesh(verts, faces, poses, K, 6, 8, 0.1),
        "triangle_grid": lambda: ops.triangle_grid(verts, faces),
        "simplify_mesh": lambda: ops.simplify_mesh(verts, faces, 0.5),
        "sample_mesh_surface": lambda: ops.sample_mesh_surface(verts, faces, 10.0),
        "voxelize_mesh": lambda: ops.voxelize_mesh(verts, faces, (4, 4, 4), (0, 0, 0), 0.5),
        "mesh_pseudonormals": lambda: ops.mesh_pseudonormals(verts, faces),
        "fuse_label_votes": lambda: ops.fuse_label_votes(table, vertex_id, pred),
        "fuse_label_evidence": lambda: ops.fuse_label_evidence(table, vertex_id, scores),
        "voxel_components": lambda: ops.voxel_components(torch.ones(5, 4, 3, dtype=u8)),
        "mesh_components": lambda: ops.mesh_components(adjacency),
        "component_sizes": lambda: ops.component_sizes(torch.zeros(5, dtype=i32)),
        "point_grid": lambda: ops.point_grid(verts),
        "nearest_point": lambda: ops.nearest_point(grid, verts, 0.5),
    }


# Ops that reached lib() before rejecting CPU tensors when ops was one file would be
# listed here and excused from that half of the assertion; there was none.
REACHED_LIBRARY_BEFORE = frozenset()


@pytest.fixture
def no_library(monkeypatch):
    def boom(*a, **k):
        raise ReachedLibrary("the op reached lib() with CPU tensors")
    mods = [ops] + [m for m in vars(ops).values()
                    if inspect.ismodule(m) and m.__name__.startswith(ops.__name__ + ".")]
    for m in mods:
        if hasattr(m, "lib"):
            monkeypatch.setattr(m, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("name", sorted(_cpu_calls()))
def test_cpu_tensors_are_rejected_before_the_library(name, no_library):
    call = _cpu_calls()[name]
    if name in REACHED_LIBRARY_BEFORE:
        with pytest.raises((_lib.UcsaError, ReachedLibrary)):
            call()
        return
    with pytest.raises(_lib.UcsaError):
        call()


if __name__ == "__main__":      # regenerate the snapshot (from the tree it describes)
    with open(GOLDEN, "w") as fh:
        json.dump(snapshot(ops), fh, indent=1, sort_keys=True)
        fh.write("\n")
