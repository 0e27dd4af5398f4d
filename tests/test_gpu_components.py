"""GPU: connected components (csrc/components.hip: ucsa_voxel_components,
ucsa_graph_components, ucsa_component_sizes) against the numpy restatement of
their contracts (tests/components_numpy.py).  Every comparison is byte
equality: a label is the smallest index of its component.  Guard words,
unchanged inputs, repeatability, argument codes; floaters removed from a TSDF
volume (utils/tsdf_fusion.remove_small_components) and from a mesh
(utils/mesh_fusion.filter_mesh_components); the three scripts with
--min_component on an exported synthetic scene."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import components_numpy as CN
from tests.test_gpu_tsdf_fusion import _cu, _ops
from tests.test_gpu_voxel_map import guarded

pytestmark = pytest.mark.gpu

# several tiles of 4 x 4 x 64 with ragged edges; less than one tile; thin axes
LATTICES = [(37, 20, 65), (2, 2, 9), (5, 70, 3)]
BIG = LATTICES[0]
# close to the site-percolation thresholds: large, winding components
NEAR_THRESHOLD = {6: 0.32, 26: 0.10}


def lattice_masks(dims, connectivity):
    """name -> uint8 mask (values other than 1 included)"""
    g = np.random.default_rng(0)
    i, j, k = np.indices(dims)
    out = {"threshold": (g.random(dims) < NEAR_THRESHOLD[connectivity]).astype(np.uint8),
           "dense": (g.random(dims) < 0.7).astype(np.uint8) * 200,
           "ones": np.ones(dims, np.uint8), "zeros": np.zeros(dims, np.uint8),
           "checkerboard": ((i + j + k) % 2 == 0).astype(np.uint8)}
    if dims == BIG:
        out["serpentine"] = CN.serpentine(dims).astype(np.uint8) * 255
    return out


_WANT = {}


def want_labels(dims, connectivity, name):
    """the restatement's labelling, computed once and shared (read-only)"""
    key = (dims, connectivity, name)
    if key not in _WANT:
        lab = CN.voxel_components(lattice_masks(dims, connectivity)[name], connectivity)
        lab.setflags(write=False)
        _WANT[key] = lab
    return _WANT[key]


def gpu_sizes_match(labels_gpu, labels_np):
    ops = _ops()
    got = ops.component_sizes(labels_gpu)
    want = CN.component_sizes(labels_np)
    assert got.dtype == torch.int32 and tuple(got.shape) == labels_np.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(ops.component_sizes(labels_gpu), got)          # twice: the same bytes
    assert labels_gpu.cpu().numpy().tobytes() == labels_np.tobytes()  # the input is untouched


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("dims", LATTICES)
def test_lattice_labels_and_sizes_byte_equal(dims, connectivity):
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    masks = lattice_masks(dims, connectivity)
    if dims == BIG:
        # conditions on the input: a component larger than a tile, many components
        sizes = CN.component_sizes(want_labels(dims, connectivity, "threshold"))
        lab = want_labels(dims, connectivity, "threshold")
        assert sizes.max() > 256 and len(np.unique(lab[lab >= 0])) >= 50
        lab = want_labels(dims, connectivity, "serpentine")
        assert (lab[masks["serpentine"] != 0] == 0).all() and (lab >= 0).sum() > 10000
    for name, m in masks.items():
        want = want_labels(dims, connectivity, name)
        mask = _cu(m)
        out, check = guarded(dims, torch.int32, 12345)
        assert l.ucsa_voxel_components(p(mask), p(out), *dims, connectivity, None) == 0
        torch.cuda.synchronize()
        check()
        assert out.cpu().numpy().tobytes() == want.tobytes(), name
        assert mask.cpu().numpy().tobytes() == m.tobytes(), name       # the input is untouched
        got = ops.voxel_components(mask, connectivity)                 # through ops: twice
        assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes(), name
        as_bool = ops.voxel_components(mask != 0, connectivity)
        assert torch.equal(as_bool, got), name
        gpu_sizes_match(got, want)
    assert torch.equal(ops.voxel_components(mask), ops.voxel_components(mask, 26))


def test_sizes_one_root_negative_labels_and_guards():
    from ucsa_neural_rendering_amd import _lib
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    # the full lattice: one root for every voxel, maximal contention
    full = np.array(want_labels(BIG, 26, "ones"))
    assert (full == 0).all()
    # a label array with -1s, many small labels and one large one
    g = np.random.default_rng(3)
    mixed = g.integers(-1, 40, 5001).astype(np.int32)
    mixed[1000:3000] = 4321
    for lab in (full, mixed):
        n = lab.size
        src = _cu(lab)
        sizes, check_s = guarded(lab.shape, torch.int32, -5)
        scratch, check_w = guarded((n,), torch.int32, -5)
        assert l.ucsa_component_sizes(p(src), p(sizes), p(scratch), n, None) == 0
        torch.cuda.synchronize()
        check_s()
        check_w()
        want = CN.component_sizes(lab)
        assert sizes.cpu().numpy().tobytes() == want.tobytes()
        assert src.cpu().numpy().tobytes() == lab.tobytes()
        counts = np.bincount(lab[lab >= 0].reshape(-1), minlength=n).astype(np.int32)
        assert scratch.cpu().numpy().tobytes() == counts.tobytes()
    assert int(CN.component_sizes(full)[0, 0, 0]) == full.size
    gpu_sizes_match(_cu(mixed), mixed)


def graph_cases():
    """name -> (faces [F,3] int32, V); every graph goes through ops.mesh_adjacency"""
    g = np.random.default_rng(1)
    cases = {}
    # a path of 5000 vertices under a random renumbering (degenerate faces a, b, b)
    perm = g.permutation(5000)
    cases["path"] = (np.stack([perm[:-1], perm[1:], perm[1:]], 1), 5000)
    # 300 small components of 2..7 vertices plus 50 isolated vertices, renumbered at random
    ks = g.integers(2, 8, 300)
    total = int(ks.sum()) + 50
    perm = g.permutation(total)
    faces, at = [], 0
    for k in ks:
        grp = perm[at:at + k]
        at += int(k)
        faces += [(grp[i], grp[i + 1], grp[int(g.integers(0, k))]) for i in range(k - 1)]
    cases["small"] = (np.array(faces), total)
    # a star with 4000 leaves whose centre has the largest index
    leaves = np.arange(4000)
    cases["star"] = (np.stack([np.full(4000, 4000), leaves, leaves], 1), 4001)
    cases["no_edges"] = (np.zeros((0, 3), np.int64), 7)
    cases["empty"] = (np.zeros((0, 3), np.int64), 0)
    return {k: (f.astype(np.int32), V) for k, (f, V) in cases.items()}


def two_sphere_mesh():
    """the marching-cubes mesh (all cells valid) of two disjoint spheres in 24^3"""
    ops = _ops()
    q = np.stack(np.meshgrid(*[np.arange(24, dtype=np.float32)] * 3, indexing="ij"), -1)
    f = np.maximum(5.3 - np.linalg.norm(q - np.float32([7, 8, 8]), axis=-1),
                   3.4 - np.linalg.norm(q - np.float32([17, 16, 15]), axis=-1)).astype(np.float32)
    verts, faces, normals = ops.marching_cubes(
        _cu(f), 0.0, valid=torch.ones(f.shape, dtype=torch.bool, device="cuda"))
    return verts, faces, normals


def test_graph_labels_and_sizes_byte_equal():
    from ucsa_neural_rendering_amd import _lib
    ops = _ops()
    l = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None
    for name, (faces, V) in graph_cases().items():
        off, nbr = ops.mesh_adjacency(_cu(faces).view(-1, 3), V)
        want_off, want_nbr = CN.mesh_adjacency(faces, V)
        assert off.cpu().numpy().tobytes() == want_off.tobytes()
        want = CN.graph_components(want_off, want_nbr)
        keep = (off.clone(), nbr.clone())
        out, check = guarded((V,), torch.int32, 12345)
        assert l.ucsa_graph_components(p(off), p(nbr), V, nbr.numel(), p(out), None) == 0
        torch.cuda.synchronize()
        check()
        assert out.cpu().numpy().tobytes() == want.tobytes(), name
        got = ops.mesh_components((off, nbr))
        assert got.dtype == torch.int32 and got.cpu().numpy().tobytes() == want.tobytes(), name
        assert torch.equal(off, keep[0]) and torch.equal(nbr, keep[1])  # inputs untouched
        if V:
            gpu_sizes_match(got, want)
        else:
            assert ops.component_sizes(got).numel() == 0
        if name == "path":
            assert (want == 0).all()
        if name == "small":
            assert len(np.unique(want)) == 350 and int((np.diff(want_off) == 0).sum()) == 50
        if name == "star":
            assert (want == 0).all() and np.diff(want_off)[4000] == 4000
        if name == "no_edges":
            assert want.tolist() == list(range(7))
    verts, faces, _ = two_sphere_mesh()
    V = verts.shape[0]
    adj = ops.mesh_adjacency(faces, V)
    got = ops.mesh_components(adj).cpu().numpy()
    want = CN.graph_components(*CN.mesh_adjacency(faces.cpu().numpy(), V))
    assert got.tobytes() == want.tobytes() and len(np.unique(got)) == 2 and V > 500
    gpu_sizes_match(_cu(got), want)


def test_argument_codes_through_ctypes_and_errors_from_ops():
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    l = _lib.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dims = (5, 70, 3)
    n = int(np.prod(dims))
    mask = torch.ones(dims, dtype=torch.uint8, device="cuda")
    lab, check = guarded(dims, torch.int32, 99)

    def vox(m=mask, o=lab, d=dims, c=26):
        return l.ucsa_voxel_components(p(m), p(o), d[0], d[1], d[2], c, None)
    for rc, arg in ((vox(m=None), 0), (vox(o=None), 1), (vox(o=mask), 1), (vox(d=(0, 70, 3)), 2),
                    (vox(d=(2048, 2048, 2048)), 2), (vox(d=(5, 0, 3)), 3), (vox(d=(5, 70, 0)), 4),
                    (vox(d=(262144, 1, 1)), 2), (vox(d=(1, 262144, 1)), 3), (vox(c=18), 5),
                    (vox(c=0), 5)):
        assert rc == -(1000 + arg), (rc, arg)
    off = _cu(np.array([0, 1, 2], np.int32))
    nbr = _cu(np.array([1, 0], np.int32))
    out2, check2 = guarded((2,), torch.int32, 99)

    def gra(o=off, nb=nbr, V=2, E=2, out=out2):
        return l.ucsa_graph_components(p(o), p(nb), V, E, p(out), None)
    for rc, arg in ((gra(o=None), 0), (gra(nb=None), 1), (gra(out=None), 4), (gra(out=off), 4),
                    (gra(V=2 ** 31), 2), (gra(E=2 ** 31), 3)):
        assert rc == -(1000 + arg), (rc, arg)
    assert gra(V=0, o=None, nb=None, out=None, E=0) == 0      # legal: launches nothing
    lab1 = _cu(np.zeros(n, np.int32))
    siz, check3 = guarded((n,), torch.int32, 99)
    scr, check4 = guarded((n,), torch.int32, 99)

    def siz_rc(a=lab1, b=siz, c=scr, k=n):
        return l.ucsa_component_sizes(p(a), p(b), p(c), k, None)
    for rc, arg in ((siz_rc(a=None), 0), (siz_rc(b=None), 1), (siz_rc(c=None), 2),
                    (siz_rc(b=lab1), 1), (siz_rc(c=lab1), 2), (siz_rc(c=siz), 2),
                    (siz_rc(k=2 ** 31), 3)):
        assert rc == -(1000 + arg), (rc, arg)
    assert siz_rc(a=None, b=None, c=None, k=0) == 0
    torch.cuda.synchronize()
    for c in (check, check2, check3, check4):
        c()
    # an argument error launches nothing: the outputs still hold their fill
    assert (lab == 99).all() and (out2 == 99).all() and (siz == 99).all() and (scr == 99).all()
    adj = (off, nbr)
    for bad in (lambda: ops.voxel_components(mask.cpu()),
                lambda: ops.voxel_components(mask.float()),
                lambda: ops.voxel_components(mask[0]),
                lambda: ops.voxel_components(mask, connectivity=18),
                lambda: ops.voxel_components(mask, connectivity=True),
                lambda: ops.voxel_components(mask[:, :0]),
                lambda: ops.mesh_components(off),
                lambda: ops.mesh_components((off.long(), nbr)),
                lambda: ops.mesh_components((off.cpu(), nbr)),
                lambda: ops.mesh_components((off[:0], nbr)),
                lambda: ops.mesh_components((off, nbr.view(1, 2))),
                lambda: ops.component_sizes(lab1.long()),
                lambda: ops.component_sizes(lab1.cpu())):
        with pytest.raises(UcsaError):
            bad()
    assert ops.mesh_components(adj).tolist() == [0, 0]
    # non-contiguous inputs are read as they are given
    wide = torch.ones((5, 70, 6), dtype=torch.uint8, device="cuda")
    assert torch.equal(ops.voxel_components(wide[:, :, ::2]), ops.voxel_components(mask))


# ---- the volume: a floater in observed free space ---------------------------
BLOB = (47, 57, 52)      # centre of the 3 x 3 x 3 blob, lattice coordinates


@pytest.fixture(scope="module")
def room():
    from tests import tsdf_numpy as TN
    from tests.test_tsdf_fusion_cpu import room_frames, room_volume_spec
    _, poses, intr, depth = room_frames(120, 160)                 # the smallest size of
    dims, origin, h, trunc = room_volume_spec(96)                 # tests/test_tsdf_fusion_cpu.py
    ref = TN.new_volume(dims, origin, h)
    TN.integrate(ref, depth, poses, intr, trunc)
    return {"poses": poses, "intr": intr, "depth": depth, "dims": dims, "origin": origin,
            "h": float(h), "trunc": float(trunc), "ref": ref}


def integrate_room(room):
    ops = _ops()
    vol = ops.tsdf_volume(room["dims"], room["origin"], room["h"], with_color=True)
    col = torch.full(room["depth"].shape + (3,), 90, dtype=torch.uint8, device="cuda")
    ops.integrate_tsdf(vol, _cu(room["depth"]), _cu(room["poses"]), room["intr"], room["trunc"],
                       color=col)
    return vol


def volume_bytes(vol):
    return {k: vol[k].cpu().numpy().tobytes() for k in ("tsdf", "weight", "rgb")}


def test_floater_in_free_space_is_removed_from_volume_mesh_and_raycast(room):
    """A 3 x 3 x 3 blob written into observed free space of the integrated room is
    removed: the volume, its mesh and a ray-cast view that looks at the blob are
    those of the clean volume byte for byte, the blob's own 27 voxels apart, which
    end unobserved (weight 0, rgb 0) where the clean volume had seen free space."""
    from tests.test_tsdf_fusion_cpu import look_at
    from ucsa_neural_rendering_amd.utils.tsdf_fusion import (band_mask, extract_mesh,
                                                              remove_small_components)
    ops = _ops()
    ref = room["ref"]
    band = CN.band_mask(ref)
    i, j, k = BLOB
    blob = (slice(i - 1, i + 2), slice(j - 1, j + 2), slice(k - 1, k + 2))
    # preconditions, from the restatement: the blob lies in observed free space,
    # at least 3 voxels from any band voxel, and the room's band has no
    # component under 28 voxels
    assert (ref["weight"][blob] >= 1).all() and (ref["tsdf"][blob] == 1).all()
    assert not band[i - 4:i + 5, j - 4:j + 5, k - 4:k + 5].any()
    sizes = CN.component_sizes(CN.voxel_components(band, 26))
    assert sizes[band].min() >= 28

    clean = integrate_room(room)
    assert band_mask(clean).cpu().numpy().tobytes() == band.tobytes()
    want = volume_bytes(clean)
    st = remove_small_components(clean, min_voxels=28)
    assert st["removed_components"] == 0 and st["removed_voxels"] == 0
    assert st["largest"] == int(sizes.max()) and st["components"] == 1
    assert volume_bytes(clean) == want                          # nothing under 28: no change
    mesh_clean = [t.cpu().numpy() for t in extract_mesh(clean)]

    dirty = integrate_room(room)
    dirty["tsdf"][blob] = -0.5
    dirty["weight"][blob] = 2.0
    dirty["rgb"][blob] = torch.tensor([10.0, 200.0, 30.0], device="cuda")
    mesh_dirty = [t.cpu().numpy() for t in extract_mesh(dirty)]
    assert mesh_dirty[0].shape[0] > mesh_clean[0].shape[0]

    # a view that looks at the blob from a camera whose central ray goes on to a wall
    centre = np.asarray(room["origin"], np.float64) + np.asarray(BLOB) * room["h"]
    pose = _cu(look_at(room["poses"][2][:3, 3], centre)[None])
    H, W = 60, 80
    intr = (0.89 * W, 0.89 * W, W / 2.0, H / 2.0)
    cast = lambda v: ops.raycast_tsdf(v, pose, intr, H, W, 0.05, 12.0, trunc=room["trunc"])
    depth_clean = cast(clean)["depth"]
    depth_dirty = cast(dirty)["depth"]
    mid = (0, H // 2, W // 2)
    assert 0 < depth_dirty[mid] < depth_clean[mid]              # the ray-caster hits the blob

    copy = {k: v.clone() if torch.is_tensor(v) else v for k, v in dirty.items()}
    want_np = {k: dirty[k].cpu().numpy() for k in ("tsdf", "weight", "rgb")}
    st = remove_small_components(dirty, min_voxels=28)
    want_st = CN.remove_small_components(want_np, 28)
    assert st == want_st
    assert st["removed_components"] == 1 and st["removed_voxels"] == 27 and st["components"] == 2
    assert volume_bytes(dirty) == {k: want_np[k].tobytes() for k in want_np}
    # The clean volume again, byte for byte -- except that the 27 voxels, which the
    # clean volume had observed as free space (weight >= 1, its colour), are now in
    # the volume's empty state (weight 0, rgb 0), as the contract says: what a view
    # once saw there is not known to the clean-up.
    assert dirty["tsdf"].cpu().numpy().tobytes() == want["tsdf"]
    for k in ("weight", "rgb"):
        assert (dirty[k][blob] == 0).all()
        dirty[k][blob] = clean[k][blob]
    assert volume_bytes(dirty) == want
    for k in ("weight", "rgb"):
        dirty[k][blob] = 0.0
    for a, b in zip([t.cpu().numpy() for t in extract_mesh(dirty)], mesh_clean):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert torch.equal(cast(dirty)["depth"], depth_clean)
    # connectivity 6 and a threshold the blob passes
    copy_np = {k: copy[k].cpu().numpy() for k in ("tsdf", "weight", "rgb")}
    want_st = CN.remove_small_components(copy_np, 27, connectivity=6)   # before the in-place call
    assert remove_small_components(copy, min_voxels=27, connectivity=6) == want_st
    assert volume_bytes(copy) == {k: copy_np[k].tobytes() for k in copy_np}
    assert (copy["weight"][blob] == 2).all()
    assert remove_small_components(copy, min_voxels=0)["removed_voxels"] == 0


def test_filter_mesh_components_against_the_restatement():
    from ucsa_neural_rendering_amd.utils.mesh_fusion import filter_mesh_components
    verts, faces, normals = two_sphere_mesh()
    g = np.random.default_rng(2)
    V = verts.shape[0]
    perm = g.permutation(faces.shape[0])                       # faces in no particular order
    mesh = {"verts": verts.cpu().numpy(), "faces": faces.cpu().numpy()[perm],
            "normals": normals.cpu().numpy(), "rgb": g.random((V, 3)).astype(np.float32),
            "labels": g.integers(0, 41, V).astype(np.int32), "note": "kept"}
    sizes = np.unique(CN.graph_components(*CN.mesh_adjacency(mesh["faces"], V)),
                      return_counts=True)[1]
    assert len(sizes) == 2 and sizes.min() < sizes.max()
    between = int(sizes.min()) + 1
    for kw in (dict(min_vertices=between), dict(keep_largest=1), dict(min_vertices=0),
               dict(keep_largest=2), dict(min_vertices=int(sizes.max()) + 1)):
        got, st = filter_mesh_components(mesh, **kw)
        want, want_st = CN.filter_mesh_components(mesh, **kw)
        assert st == want_st, kw
        assert sorted(got) == sorted(want)
        for k in ("verts", "faces", "normals", "rgb", "labels", "vertex_index", "face_index"):
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (kw, k)
        assert got["note"] == "kept"
    got, st = filter_mesh_components(mesh, min_vertices=between)
    assert st == {"components": 2, "removed_components": 1,
                  "removed_vertices": int(sizes.min()), "largest": int(sizes.max())}
    assert got["verts"].shape[0] == sizes.max() and got["faces"].max() == sizes.max() - 1
    bare = {"verts": mesh["verts"], "faces": mesh["faces"], "labels": None, "rgb": None}
    got, _ = filter_mesh_components(bare, keep_largest=1)
    assert got["labels"] is None and got["rgb"] is None and "normals" not in got


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_scripts_min_component_zero_changes_no_byte_and_positive_reports(tmp_path, capsys):
    """the scene and sizes of tests/test_gpu_table_smooth.py's script test"""
    from scripts import fuse_mesh_labels, fuse_tsdf_mesh, voxel_map_labels
    from ucsa_neural_rendering_amd.dataset.synthetic_export import export
    from ucsa_neural_rendering_amd.utils.ply import read_ply
    Hs, Ws, n = 240, 320, 8
    ds, sroot = export(str(tmp_path), scene_seed=0, n_views=n, H=Hs, W=Ws)
    stems = [f"{b:06d}" for b in range(n)]
    h = 6.1 / 63
    box = ["--voxel", repr(h), "--aabb", "-3.05", "-3.05", "-3.05", "3.05", "3.05", "3.05"]
    read = lambda path: open(path, "rb").read()

    def stats_line():
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("components: ")]
        return [json.loads(ln[len("components: "):]) for ln in lines]

    # TSDF mesh
    tsdf = ["--scene_root", sroot] + box
    capsys.readouterr()
    r = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "t.ply")])
    r0 = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "t0.ply"), "--min_component", "0"])
    assert stats_line() == [] and "components" not in r0
    assert read(tmp_path / "t0.ply") == read(tmp_path / "t.ply")
    for conn in ("26", "6"):
        rp = fuse_tsdf_mesh.main(tsdf + ["--out", str(tmp_path / "tp.ply"), "--min_component",
                                         "50", "--component_connectivity", conn])
        (st,) = stats_line()
        assert st == rp["components"] and st["components"] >= 1 and st["largest"] >= 50
        assert 0 < rp["vertices"] <= r["vertices"]
        assert read_ply(str(tmp_path / "tp.ply"))["verts"].shape[0] == rp["vertices"]
    # voxel map
    vox = ["--scene_root", sroot, "--labels", "label_40", "--step", repr(0.5 * h)] + box
    voxel_map_labels.main(vox + ["--out_dir", str(tmp_path / "v")])
    v0 = voxel_map_labels.main(vox + ["--out_dir", str(tmp_path / "v0"), "--min_component", "0"])
    assert stats_line() == [] and "components" not in v0
    vp = voxel_map_labels.main(vox + ["--out_dir", str(tmp_path / "vp"), "--min_component", "50",
                                      "--component_connectivity", "6"])
    (st,) = stats_line()
    assert st == vp["components"] and st["largest"] >= 50
    for s in stems:
        for k in ("map_label", "map_depth"):
            assert read(tmp_path / "v0" / k / (s + ".png")) == read(tmp_path / "v" / k / (s + ".png"))
            assert _png(tmp_path / "vp" / k / (s + ".png")).shape == (Hs, Ws)
    # labels fused onto the TSDF mesh
    fus = ["--scene_root", sroot, "--mesh", str(tmp_path / "t.ply"), "--labels", "label_40",
           "--render"]
    fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "f.ply"), "--out_dir", str(tmp_path / "m")])
    f0 = fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "f0.ply"), "--out_dir",
                                      str(tmp_path / "m0"), "--min_component", "0"])
    assert stats_line() == [] and "components" not in f0
    assert read(tmp_path / "f0.ply") == read(tmp_path / "f.ply")
    fp = fuse_mesh_labels.main(fus + ["--out", str(tmp_path / "fp.ply"), "--out_dir",
                                      str(tmp_path / "mp"), "--min_component", "50"])
    (st,) = stats_line()
    assert st == fp["components"] and st["largest"] >= 50
    ply = read_ply(str(tmp_path / "fp.ply"))
    assert ply["verts"].shape[0] == fp["vertices"] == r["vertices"] - st["removed_vertices"]
    assert ply["faces"].max() < fp["vertices"] and "labels" in ply and "normals" in ply
    for s in stems:
        assert read(tmp_path / "m0" / "map_label" / (s + ".png")) == \
            read(tmp_path / "m" / "map_label" / (s + ".png"))
        assert _png(tmp_path / "mp" / "map_label" / (s + ".png")).shape == (Hs, Ws)
