"""TSDF volumes: fusion, the occupancy prior, per-voxel votes and evidence,
the ray-caster, table smoothing and voxel components."""
from __future__ import annotations

import math
from typing import Optional

import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import (_cameras, _centre, _class_planes, _count, _gpu, _non_negative,
                    _origin_spacing, _positive, _ptr, _scratch_named, _stream, _views,
                    volume_lattice)


# ---------------------------------------------------------------------------
# TSDF fusion (posed depth frames into a dense volume)
# ---------------------------------------------------------------------------
def tsdf_volume(dims, origin, spacing, with_color: bool = False, device="cuda"):
    """An empty TSDF volume for ``integrate_tsdf``: dict with ``tsdf`` [nx,ny,nz]
    f32 (ones: free), ``weight`` [nx,ny,nz] f32 (zeros: unobserved), ``rgb``
    [nx,ny,nz,3] f32 (zeros) or None, and the lattice ``origin`` / ``spacing``
    (3 floats each; point (i,j,k) at origin + (i,j,k)*spacing, poses' frame,
    scene units)."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7FFFFFFF:
        raise _lib.UcsaError(f"tsdf_volume: dims must be >= 2 each with at most 2^31-1 "
                             f"voxels, got {(nx, ny, nz)}")
    spacing = [float(spacing)] * 3 if isinstance(spacing, (int, float)) else \
        [float(v) for v in spacing]
    origin = [float(v) for v in origin]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError("tsdf_volume: origin and spacing have 3 entries each")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.UcsaError("tsdf_volume: the volume lives on the GPU (no CPU fallback)")
    return {"tsdf": torch.ones(nx, ny, nz, device=dev),
            "weight": torch.zeros(nx, ny, nz, device=dev),
            "rgb": torch.zeros(nx, ny, nz, 3, device=dev) if with_color else None,
            "origin": tuple(origin), "spacing": tuple(spacing)}


def integrate_tsdf(volume, depth, poses, intrinsics, trunc: float, color=None,
                   max_weight: float = 65504.0, depth_min: float = 1e-6,
                   depth_max: float = 3.0e38):
    """Integrate B posed depth views into ``volume`` (``tsdf_volume``), in place;
    returns ``volume``.  ``depth`` [B,H,W] f32 z-depth in scene units (0, NaN,
    inf, anything outside [depth_min, depth_max] = no measurement), ``poses``
    [B,4,4] camera-to-world in the volume's frame, ``intrinsics`` (fx, fy, cx,
    cy) as for get_rays, ``trunc`` the truncation distance in scene units,
    ``color`` [B,H,W,3] uint8 iff the volume has ``rgb``.  Contract of
    ucsa_tsdf_integrate (include/ucsa_hip.h): a voxel's views are applied in
    order, so any split of the views over calls gives the same bytes."""
    (nx, ny, nz), dev = volume_lattice(volume)
    tsdf, weight, rgb = volume["tsdf"], volume["weight"], volume.get("rgb")
    depth, poses, (B, H, W), (fx, fy, cx, cy) = _views(depth, poses, intrinsics, dev)
    if (color is None) != (rgb is None):
        raise _lib.UcsaError("color frames and a colour volume come as a pair")
    if color is not None:
        color = _gpu(color, "color", torch.uint8, (B, H, W, 3), device=dev)
    check(lib().ucsa_tsdf_integrate(
        _ptr(tsdf), _ptr(weight), _ptr(rgb), nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(color), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(max_weight), float(depth_min), float(depth_max),
        _stream()), "ucsa_tsdf_integrate")
    return volume


def tsdf_occupancy(volume, bound, cascade=None, H: int = 128, dilate=None,
                   min_weight: float = 1.0, free_tsdf: float = 1.0, unknown: str = "keep"):
    """Occupancy prior of a ``tsdf_volume`` for the marcher's cascade grid:
    uint8 [cascade,H,H,H] on the volume's device, 1 = the cell may hold matter,
    0 = every voxel its box meets was seen to be free space
    (``weight >= min_weight and tsdf >= free_tsdf``).  ``cascade`` None is the
    renderer's ``1 + ceil(log2(bound))``; ``dilate`` (scene units, grows every
    cell's box on all sides) None is the largest of the three spacings: one
    voxel, because the voxels that no view observed next to a surface hold no
    evidence either way; ``unknown`` "keep" keeps every cell that touches an
    unobserved voxel or reaches outside the volume, "empty" carves them.
    ``SemanticNeRFRenderer.set_occupancy_prior`` takes the result.  Contract of
    ucsa_tsdf_occupancy (include/ucsa_hip.h): a pure OR over a box of voxels,
    the same bytes every run."""
    (nx, ny, nz), dev = volume_lattice(volume)
    if unknown not in ("keep", "empty"):
        raise _lib.UcsaError(f"tsdf_occupancy: unknown must be 'keep' or 'empty', got {unknown!r}")
    bound = _positive(bound, "tsdf_occupancy: bound")
    if cascade is None:
        cascade = 1 + math.ceil(math.log2(bound))
    cascade, H = int(cascade), int(H)
    if not 1 <= cascade <= 31:
        raise _lib.UcsaError(f"tsdf_occupancy: cascade must be in 1..31, got {cascade}")
    if not 2 <= H <= 1024:
        raise _lib.UcsaError(f"tsdf_occupancy: H must be in 2..1024, got {H}")
    origin, spacing = _origin_spacing("tsdf_occupancy", volume["origin"], volume["spacing"])
    dilate = _non_negative(max(spacing) if dilate is None else dilate, "tsdf_occupancy: dilate")
    if math.isnan(float(min_weight)) or math.isnan(float(free_tsdf)):
        raise _lib.UcsaError("tsdf_occupancy: min_weight and free_tsdf must not be NaN")
    mask = torch.empty(cascade, H, H, H, dtype=torch.uint8, device=dev)
    ws_bytes = int(lib().ucsa_tsdf_occupancy_workspace_bytes(nx, ny, nz))
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    check(lib().ucsa_tsdf_occupancy(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), nx, ny, nz, fvec(origin), fvec(spacing),
        float(min_weight), float(free_tsdf), 1 if unknown == "keep" else 0, bound, cascade, H,
        dilate, _ptr(mask), mask.numel(), _ptr(ws), ws_bytes, _stream()), "ucsa_tsdf_occupancy")
    return mask


# ---------------------------------------------------------------------------
# voxel map (per-voxel class votes, ray-caster over the TSDF volume)
# ---------------------------------------------------------------------------
def _new_class_table(what, volume, n_classes, dtype):
    (nx, ny, nz), dev = volume_lattice(volume)
    Cn = int(n_classes)
    if not 1 <= Cn <= 255:
        raise _lib.UcsaError(f"{what}: n_classes must be in 1..255, got {n_classes}")
    if (Cn + 1) * nx * ny * nz > 1 << 40:
        raise _lib.UcsaError(f"{what}: (C+1)*nx*ny*nz must be at most 2^40")
    return torch.zeros(Cn + 1, nx, ny, nz, dtype=dtype, device=dev)


def voxel_votes(volume, n_classes: int):
    """The zeroed vote table of a ``tsdf_volume`` for ``vote_voxel_labels``:
    [C+1, nx, ny, nz] uint16, class-major (plane = class id, plane 0 unused),
    1 <= C <= 255."""
    return _new_class_table("voxel_votes", volume, n_classes, torch.uint16)


def vote_voxel_labels(votes, volume, depth, pred, poses, intrinsics, trunc: float,
                      depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """B posed views vote into ``votes`` (``voxel_votes``), in place; returns
    ``votes``.  ``depth`` [B,H,W] f32, ``poses`` [B,4,4], ``intrinsics`` as for
    ``integrate_tsdf``; ``pred`` [B,H,W] uint8 class ids.  A voxel votes for
    pred's class at the pixel it projects to iff the depth there puts it in the
    band |z - c_z| <= trunc and 1 <= pred <= C; counts saturate at 65535.
    Contract of ucsa_tsdf_vote (include/ucsa_hip.h): independent of the TSDF
    state, and the same bytes for every split and order of the views."""
    (nx, ny, nz), dev = volume_lattice(volume)
    Cn = _class_planes(votes, "votes", torch.uint16, (nx, ny, nz), dev)
    depth, poses, (B, H, W), (fx, fy, cx, cy) = _views(depth, poses, intrinsics, dev)
    pred = _gpu(pred, "pred", torch.uint8, (B, H, W), device=dev)
    check(lib().ucsa_tsdf_vote(
        _ptr(votes), votes.numel(), Cn, nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(pred), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(depth_min), float(depth_max), _stream()), "ucsa_tsdf_vote")
    return votes


def resolve_voxel_labels(votes, min_votes: int = 1):
    """``votes`` [C+1,nx,ny,nz] -> dict of device tensors [nx,ny,nz]: ``label``
    uint8 (the class with the most votes, ties to the lower id, 0 where the
    voxel's total is below ``min_votes``), ``total`` and ``winner`` uint32
    (confidence = winner / total).  ucsa_voxel_label_resolve."""
    Cn = _class_planes(votes, "votes", torch.uint16)
    min_votes = int(min_votes)
    if not 1 <= min_votes < 1 << 32:
        raise _lib.UcsaError(f"min_votes must be in 1..2^32-1, got {min_votes}")
    shape, dev = tuple(votes.shape[1:]), votes.device
    n = int(votes[0].numel())
    out = {"label": torch.empty(shape, dtype=torch.uint8, device=dev),
           "total": torch.empty(shape, dtype=torch.uint32, device=dev),
           "winner": torch.empty(shape, dtype=torch.uint32, device=dev)}
    check(lib().ucsa_voxel_label_resolve(_ptr(votes), Cn, n, min_votes, _ptr(out["label"]),
                                         _ptr(out["total"]), _ptr(out["winner"]), n,
                                         _stream()), "ucsa_voxel_label_resolve")
    return out


def voxel_evidence(volume, n_classes: int):
    """The zeroed evidence table of a ``tsdf_volume`` for
    ``accumulate_voxel_evidence``: [C+1, nx, ny, nz] uint32, class-major; plane
    c (1..C) is the evidence sum of class c, plane 0 the number of (view,
    voxel) contributions.  Limits as for ``voxel_votes``."""
    return _new_class_table("voxel_evidence", volume, n_classes, torch.uint32)


def accumulate_voxel_evidence(evidence, volume, depth, scores, poses, intrinsics, trunc: float,
                              depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """The soft form of ``vote_voxel_labels``: B posed views add evidence into
    ``evidence`` (``voxel_evidence``), in place; returns ``evidence``.
    ``depth`` [B,H,W] f32, ``poses`` [B,4,4], ``intrinsics`` as for
    ``integrate_tsdf``; ``scores`` [B,H,W,C] uint8 (``log_evidence``).  A voxel
    takes the row of the pixel it projects to under exactly the rule of
    ``vote_voxel_labels`` (the band |z - c_z| <= trunc) unless the row is all
    zero, adds it to its C planes and 1 to plane 0; all adds saturate at
    2^32-1.  A voxel that no view of the call reaches is neither read nor
    written.  Contract of ucsa_tsdf_evidence (include/ucsa_hip.h): independent
    of the TSDF state, and the same bytes for every split and order of the
    views."""
    (nx, ny, nz), dev = volume_lattice(volume)
    Cn = _class_planes(evidence, "evidence", torch.uint32, (nx, ny, nz), dev)
    depth, poses, (B, H, W), (fx, fy, cx, cy) = _views(depth, poses, intrinsics, dev)
    scores = _gpu(scores, "scores", torch.uint8, (B, H, W, Cn), device=dev)
    check(lib().ucsa_tsdf_evidence(
        _ptr(evidence), evidence.numel(), Cn, nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(scores), _ptr(poses), B, fx, fy, cx, cy,
        H, W, float(trunc), float(depth_min), float(depth_max), _stream()),
        "ucsa_tsdf_evidence")
    return evidence


def resolve_voxel_evidence(evidence, min_views: int = 1, min_margin: int = 0):
    """``evidence`` [C+1,nx,ny,nz] -> dict of device tensors [nx,ny,nz]:
    ``label`` uint8 (the class with the largest evidence sum, ties to the lower
    id, 0 where plane 0 < ``min_views`` or margin < ``min_margin``), ``views``
    (plane 0), ``best`` and ``margin`` uint32 (best minus the runner-up; for
    C = 1 it is best).  ``label`` feeds ``raycast_tsdf(voxel_labels=...)``.
    ucsa_voxel_evidence_resolve."""
    Cn = _class_planes(evidence, "evidence", torch.uint32)
    min_views, min_margin = int(min_views), int(min_margin)
    if not 1 <= min_views < 1 << 32:
        raise _lib.UcsaError(f"min_views must be in 1..2^32-1, got {min_views}")
    if not 0 <= min_margin < 1 << 32:
        raise _lib.UcsaError(f"min_margin must be in 0..2^32-1, got {min_margin}")
    shape, dev = tuple(evidence.shape[1:]), evidence.device
    n = int(evidence[0].numel())
    out = {"label": torch.empty(shape, dtype=torch.uint8, device=dev),
           "views": torch.empty(shape, dtype=torch.uint32, device=dev),
           "best": torch.empty(shape, dtype=torch.uint32, device=dev),
           "margin": torch.empty(shape, dtype=torch.uint32, device=dev)}
    check(lib().ucsa_voxel_evidence_resolve(
        _ptr(evidence), Cn, n, min_views, min_margin, _ptr(out["label"]), _ptr(out["views"]),
        _ptr(out["best"]), _ptr(out["margin"]), n, _stream()), "ucsa_voxel_evidence_resolve")
    return out


def raycast_tsdf(volume, poses, intrinsics, H: int, W: int, near: float, far: float,
                 step: Optional[float] = None, min_weight: float = 1.0, voxel_labels=None,
                 trunc: Optional[float] = None, _plain_march: bool = False):
    """The model view of a TSDF volume from B posed cameras -> dict of device
    tensors: ``depth`` [B,H,W] f32 (z-depth of the first surface along the
    pixel's ray, 0 = miss), ``voxel_id`` [B,H,W] int32 (linear index of the
    nearest lattice point, -1 = miss), ``normal`` [B,H,W,3] f32 (world frame,
    toward free space), ``rgb`` [B,H,W,3] f32 when the volume has colour,
    ``label`` [B,H,W] int32 when ``voxel_labels`` [nx,ny,nz] uint8 is given.
    ``trunc`` is the truncation distance the volume was integrated with
    (default: ``volume["trunc"]``, which utils/voxel_map.py records);
    ``step`` the march step in scene units (default trunc / 2, must stay below
    trunc); only cells whose eight corners have weight >= ``min_weight`` are
    seen (the masked mesh's cell rule).  Contract of ucsa_tsdf_raycast
    (include/ucsa_hip.h); ``_plain_march`` selects the march without
    empty-space skipping, which gives the same bytes."""
    (nx, ny, nz), dev = volume_lattice(volume)
    poses, B, (fx, fy, cx, cy) = _cameras(poses, intrinsics, dev)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise _lib.UcsaError("raycast_tsdf: H, W must be >= 1")
    if trunc is None:
        trunc = volume.get("trunc")
    if trunc is None:
        raise _lib.UcsaError("raycast_tsdf: pass trunc, the truncation distance the volume "
                             "was integrated with (or record it as volume['trunc'])")
    trunc = float(trunc)
    step = 0.5 * trunc if step is None else float(step)
    rgb = volume.get("rgb")
    labels = None if voxel_labels is None else _gpu(voxel_labels, "voxel_labels", torch.uint8,
                                                    (nx, ny, nz), device=dev)
    out = {"depth": torch.empty(B, H, W, device=dev),
           "voxel_id": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "normal": torch.empty(B, H, W, 3, device=dev)}
    if rgb is not None:
        out["rgb"] = torch.empty(B, H, W, 3, device=dev)
    if labels is not None:
        out["label"] = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    ws, ws_bytes = None, 0
    if not _plain_march:
        ws_bytes = int(lib().ucsa_tsdf_raycast_workspace_bytes(nx, ny, nz))
        ws = _scratch_named("raycast", ws_bytes, dev)
    check(lib().ucsa_tsdf_raycast(
        _ptr(volume["tsdf"]), _ptr(volume["weight"]), _ptr(rgb), _ptr(labels), nx, ny, nz,
        fvec(volume["origin"]), fvec(volume["spacing"]), _ptr(poses), B, fx, fy, cx, cy, H, W,
        float(near), float(far), trunc, step, float(min_weight), _ptr(out["depth"]),
        _ptr(out["voxel_id"]), _ptr(out["normal"]), _ptr(out.get("rgb")),
        _ptr(out.get("label")), B * H * W, _ptr(ws), ws_bytes, 1 if _plain_march else 0,
        _stream()), "ucsa_tsdf_raycast")
    return out


# ---------------------------------------------------------------------------
# neighbourhood pooling of the fused label tables
# ---------------------------------------------------------------------------
def smooth_voxel_table(table, volume, neighbourhood: int = 26, iterations: int = 1,
                       centre: int = 1, min_weight: float = 1.0):
    """Pool a voxel table over each voxel's observed neighbours -> a NEW table
    of the same dtype and shape; ``table`` is not modified.  ``table``
    [C+1,nx,ny,nz], contiguous, on the volume's device: uint32
    (``voxel_evidence``) or uint16 (``voxel_votes``).  With obs(v) =
    ``volume["weight"][v] >= min_weight`` (fp32, the ray-caster's cell rule), a
    voxel with obs(v) gets, in every plane p = 0..C,
    min(SAT, centre * table[p, v] + the sum of table[p, n]) over its 6 face
    neighbours or the 26 neighbours of the 3x3x3 cube (``neighbourhood``) that
    lie inside the lattice and have obs(n); a voxel without obs(v) keeps its
    column.  SAT is 2^32-1 / 65535.  ``iterations`` = k gives the bytes of k
    single calls.  Plane 0 of an evidence table becomes a pooled contribution
    count: ``resolve_voxel_evidence(min_views=...)`` then applies to that count,
    and ``min_margin`` / ``min_votes`` to pooled sums (up to centre + 26 times a
    single voxel's).  Contract of ucsa_voxel_table_smooth (include/ucsa_hip.h)."""
    (nx, ny, nz), dev = volume_lattice(volume)
    Cn = _class_planes(table, "table", (torch.uint32, torch.uint16), (nx, ny, nz), dev)
    if neighbourhood not in (6, 26):
        raise _lib.UcsaError(f"neighbourhood must be 6 or 26, got {neighbourhood!r}")
    centre = _centre(centre)
    _count(iterations, "iterations")
    weight = volume["weight"]
    src, spare = table, None
    for _ in range(iterations):
        dst = torch.empty_like(table) if spare is None else spare
        check(lib().ucsa_voxel_table_smooth(
            _ptr(src), _ptr(dst), table.element_size(), Cn, nx, ny, nz, _ptr(weight),
            float(min_weight), int(neighbourhood), centre, _stream()), "ucsa_voxel_table_smooth")
        # ping-pong between two fresh buffers; the input is only ever read
        spare = src if src is not table else None
        src = dst
    return src


# ---------------------------------------------------------------------------
# connected components (voxel mask, mesh graph, component sizes)
# ---------------------------------------------------------------------------
def voxel_components(mask, connectivity: int = 26):
    """Connected components of a voxel mask -> int32 [nx,ny,nz]: the smallest
    linear index ``(i*ny + j)*nz + k`` of the voxel's component where ``mask``
    is set, -1 elsewhere.  ``mask`` [nx,ny,nz] bool or uint8 (non-zero = set) on
    the GPU; it is not modified.  ``connectivity`` 6 (face neighbours) or 26
    (the 3x3x3 cube), the neighbourhoods of ``smooth_voxel_table``.  Contract of
    ucsa_voxel_components (include/ucsa_hip.h)."""
    m = _gpu(mask, "mask", (torch.bool, torch.uint8))
    if mask.dim() != 3 or mask.numel() == 0 or mask.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError(f"mask must be [nx,ny,nz] with 1 to 2^31-1 voxels, got "
                             f"{tuple(mask.shape)}")
    if isinstance(connectivity, bool) or connectivity not in (6, 26):
        raise _lib.UcsaError(f"connectivity must be 6 or 26, got {connectivity!r}")
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    nx, ny, nz = (int(s) for s in m.shape)
    labels = torch.empty((nx, ny, nz), dtype=torch.int32, device=m.device)
    check(lib().ucsa_voxel_components(_ptr(m), _ptr(labels), nx, ny, nz, int(connectivity),
                                      _stream()), "ucsa_voxel_components")
    return labels


def component_sizes(labels):
    """The size of each element's component -> int32 of ``labels``' shape:
    the number of elements that carry ``labels[x]``, 0 where ``labels[x]`` < 0.
    ``labels`` int32 on the GPU, any shape, as ``voxel_components`` /
    ``mesh_components`` give it (values below the number of elements); it is not
    modified.  Contract of ucsa_component_sizes (include/ucsa_hip.h)."""
    lab = _gpu(labels, "labels", torch.int32)
    if lab.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("labels must have at most 2^31-1 elements")
    sizes = torch.empty_like(lab)
    scratch = torch.empty_like(lab)
    check(lib().ucsa_component_sizes(_ptr(lab), _ptr(sizes), _ptr(scratch), lab.numel(),
                                     _stream()), "ucsa_component_sizes")
    return sizes
