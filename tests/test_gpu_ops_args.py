"""GPU: the conversions the shared argument checks of ops/_args.py own.  Posed
views (``_views``): a non-contiguous depth and float64 poses must give the
bytes of contiguous float32 ones.  Meshes (``_mesh``): int64 faces must give the
bytes of int32 ones, and a face index equal to V is turned away.  The shapes
are the smallest at which a wrong stride or dtype would still change bytes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS, ORIGIN, SPACING = (5, 4, 3), (-0.4, -0.3, 1.0), 0.2
B, H, W, CLASSES = 2, 6, 8, 3
K = (6.0, 6.0, 4.0, 3.0)            # the lattice fills most of the 6x8 image
TRUNC = 0.15


def _ops():
    from ucsa_neural_rendering_amd import ops
    return ops


def _poses():
    poses = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)     # camera looks down +z
    poses[1, :3, 3] = torch.tensor([0.1, 0.0, -0.1], dtype=torch.float64)
    return poses.cuda()


def _views(plain: bool):
    g = torch.Generator().manual_seed(7)
    wide = (1.0 + 0.4 * torch.rand(B, H, W + 5, generator=g)).cuda()
    pred = torch.randint(1, CLASSES + 1, (B, H, W), generator=g, dtype=torch.uint8).cuda()
    scores = torch.randint(0, 256, (B, H, W, CLASSES), generator=g, dtype=torch.uint8).cuda()
    depth, poses = wide[:, :, :W], _poses()
    assert not depth.is_contiguous() and poses.dtype == torch.float64
    if plain:
        depth, poses = depth.contiguous(), poses.float().contiguous()
    return depth, poses, pred, scores


def _fuse(plain: bool):
    ops = _ops()
    depth, poses, pred, scores = _views(plain)
    vol = ops.tsdf_volume(DIMS, ORIGIN, SPACING)
    ops.integrate_tsdf(vol, depth, poses, K, TRUNC)
    votes = ops.vote_voxel_labels(ops.voxel_votes(vol, CLASSES), vol, depth, pred, poses, K, TRUNC)
    evidence = ops.accumulate_voxel_evidence(ops.voxel_evidence(vol, CLASSES), vol, depth, scores,
                                             poses, K, TRUNC)
    torch.cuda.synchronize()
    return {"tsdf": vol["tsdf"], "weight": vol["weight"], "votes": votes.view(torch.int16),
            "evidence": evidence.view(torch.int32)}


def test_strided_depth_and_float64_poses_give_the_bytes_of_plain_views():
    want, got = _fuse(True), _fuse(False)
    for k in want:
        assert int((want[k] != 0).sum()) > 0, k               # the views reach the lattice
        assert torch.equal(want[k].view(torch.uint8), got[k].view(torch.uint8)), k


VERTS = [[-0.4, -0.3, 1.2], [0.4, -0.3, 1.2], [-0.4, 0.3, 1.3], [0.4, 0.3, 1.1]]
FACES = [[0, 1, 2], [1, 3, 2]]


def _mesh_results(faces):
    ops = _ops()
    verts = torch.tensor(VERTS, dtype=torch.float32).cuda()
    ras = ops.rasterize_mesh(verts, faces, _poses(), K, H, W, 0.1)
    vox = ops.voxelize_mesh(verts, faces, (4, 4, 4), (-0.4, -0.3, 1.0), 0.2)
    torch.cuda.synchronize()
    return dict(ras, vox=vox)


def test_int64_faces_give_the_bytes_of_int32_faces():
    want = _mesh_results(torch.tensor(FACES, dtype=torch.int32).cuda())
    got = _mesh_results(torch.tensor(FACES, dtype=torch.int64).cuda())
    assert bool((want["tri_id"] >= 0).any()) and bool((want["tri_id"] == 1).any())
    assert 0 < int(want["vox"].sum()) < want["vox"].numel()
    assert set(want) == set(got)
    for k in want:
        assert want[k].dtype == got[k].dtype, k
        assert torch.equal(want[k].view(torch.uint8), got[k].view(torch.uint8)), k


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_a_face_index_equal_to_V_is_turned_away(dtype):
    from ucsa_neural_rendering_amd._lib import UcsaError
    ops = _ops()
    verts = torch.tensor(VERTS, dtype=torch.float32).cuda()
    faces = torch.tensor([[0, 1, 2], [1, len(VERTS), 2]], dtype=dtype).cuda()
    with pytest.raises(UcsaError):
        ops.rasterize_mesh(verts, faces, _poses(), K, H, W, 0.1)
    with pytest.raises(UcsaError):
        ops.voxelize_mesh(verts, faces, (4, 4, 4), (-0.4, -0.3, 1.0), 0.2)
