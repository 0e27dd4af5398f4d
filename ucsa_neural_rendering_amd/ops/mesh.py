"""Meshes: marching cubes, the rasterizer, label fusion onto vertices, vertex
adjacency and table smoothing, components, simplification and surface samples."""
from __future__ import annotations

import ctypes as C
import math
import operator

import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import (_INTEGER, _cameras, _centre, _count, _f32, _finite_box, _gpu, _mesh,
                    _positive, _ptr, _stream)


# ---------------------------------------------------------------------------
# marching cubes (labelled-mesh export)
# ---------------------------------------------------------------------------
def marching_cubes(field, iso: float, origin=(0.0, 0.0, 0.0),
                   spacing=(1.0, 1.0, 1.0), valid=None):
    """Indexed iso-surface of a lattice field [nx,ny,nz] (point (i,j,k) at
    origin + (i,j,k)*spacing; inside iff field > iso) ->
    (verts [V,3] f32, faces [F,3] int32, normals [V,3] f32), conventions of
    ucsa_mc_count / ucsa_mc_emit (include/ucsa_hip.h).  ``valid`` [nx,ny,nz]
    bool or uint8 (a TSDF volume's observed voxels): vertices only on edges
    between two valid points, triangles only from cells with eight valid
    corners (ucsa_mc_count_masked / ucsa_mc_emit_masked); None = every point.
    Reads the two totals back once, between the passes.  Workspace: 10 bytes
    per lattice point."""
    field = _f32(field, "field")
    if field.dim() != 3:
        raise _lib.UcsaError(f"field must be [nx,ny,nz], got {tuple(field.shape)}")
    nx, ny, nz = (int(s) for s in field.shape)
    dev = field.device
    head = (_ptr(field),)
    count, emit, what = lib().ucsa_mc_count, lib().ucsa_mc_emit, "ucsa_mc"
    if valid is not None:
        if not (torch.is_tensor(valid) and valid.is_cuda):
            raise _lib.UcsaError("valid must be a GPU tensor: the HIP path has no CPU fallback")
        if valid.dtype not in (torch.bool, torch.uint8):
            raise _lib.UcsaError(f"valid must be bool or uint8, got {valid.dtype}")
        if valid.shape != field.shape or valid.device != dev:
            raise _lib.UcsaError(f"valid must be {tuple(field.shape)} on {dev}, got "
                                 f"{tuple(valid.shape)} on {valid.device}")
        valid = valid.contiguous().view(torch.uint8)
        head = (_ptr(field), _ptr(valid))
        count, emit, what = lib().ucsa_mc_count_masked, lib().ucsa_mc_emit_masked, \
            "ucsa_mc_masked"
    ws = torch.empty(int(lib().ucsa_mc_workspace_bytes(nx, ny, nz)), dtype=torch.uint8,
                     device=dev)
    totals = torch.zeros(2, dtype=torch.int32, device=dev)
    check(count(*head, nx, ny, nz, float(iso), _ptr(ws), _ptr(totals), _stream()),
          what + " count")
    V, F = (int(v) & 0xFFFFFFFF for v in totals.tolist())
    if V > 0x7FFFFFFF or F > 0x7FFFFFFF:
        raise _lib.UcsaError("marching_cubes: more than 2^31-1 vertices or triangles; "
                             "use a coarser lattice or split it")
    verts = torch.empty(V, 3, device=dev)
    normals = torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    if V or F:
        check(emit(*head, nx, ny, nz, float(iso), fvec(origin), fvec(spacing), _ptr(ws),
                   _ptr(verts), _ptr(normals), _ptr(faces), V, F, _stream()), what + " emit")
    return verts, faces, normals


# ---------------------------------------------------------------------------
# mesh rasterization (labelled meshes into camera views)
# ---------------------------------------------------------------------------
RASTER_MAX_DIM = 16384


def rasterize_mesh(verts, faces, poses, intrinsics, H: int, W: int, near: float,
                   vertex_labels=None, vertex_rgb=None):
    """A triangle mesh seen from B pinhole cameras (poses [B,4,4]
    camera-to-world in the field's frame, intrinsics (fx, fy, cx, cy): the
    conventions of get_rays) -> dict of device tensors ``tri_id`` [B,H,W] int32
    (-1 = empty), ``depth`` [B,H,W] f32 z-depth (0 = empty), ``label`` [B,H,W]
    int32 (``vertex_labels`` of the nearest corner of the hit point, 0 = empty
    or no labels) and, with ``vertex_rgb`` [V,3], ``rgb`` [B,H,W,3] f32
    (barycentric blend).  verts [V,3] f32, faces [F,3] int32 with indices in
    [0,V).  Contract of ucsa_raster_setup / ucsa_raster_draw
    (include/ucsa_hip.h): watertight, nearest face wins, ties to the lower face
    id, deterministic.  Reads back the face index range (validation) and,
    between the passes, the (tile, face) pair total."""
    verts, faces = _mesh(verts, faces, any_integer=True)
    dev = verts.device
    poses, B, (fx, fy, cx, cy) = _cameras(poses, intrinsics, dev)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    H, W = int(H), int(W)
    if not (1 <= H <= RASTER_MAX_DIM and 1 <= W <= RASTER_MAX_DIM):
        raise _lib.UcsaError(f"H, W must be in [1, {RASTER_MAX_DIM}], got {H}x{W}")
    if B > 65535 or B * F > 0x7FFFFFFF:
        raise _lib.UcsaError("rasterize_mesh: too many views x faces in one call; "
                             "render fewer views at a time")
    near = _positive(near, "near")
    labels = rgb_in = None
    if vertex_labels is not None:
        labels = _gpu(vertex_labels, "vertex_labels", shape=(V,), device=dev).to(torch.int32)
    if vertex_rgb is not None:
        rgb_in = _gpu(_f32(vertex_rgb, "vertex_rgb"), "vertex_rgb", shape=(V, 3), device=dev)
    args = (_ptr(verts), V, _ptr(faces), F, _ptr(poses), B, fx, fy, cx, cy, H, W, near)
    ws = torch.empty(int(lib().ucsa_raster_workspace_bytes(B, F, H, W)), dtype=torch.uint8,
                     device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib().ucsa_raster_setup(*args, _ptr(ws), _ptr(total), _stream()),
          "ucsa_raster_setup")
    n_pairs = int(total.item())
    if n_pairs > 0x7FFFFFFF:
        raise _lib.UcsaError("rasterize_mesh: more than 2^31-1 (tile, face) pairs; "
                             "render fewer views at a time")
    pairs = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    out = {"tri_id": torch.empty(B, H, W, dtype=torch.int32, device=dev),
           "depth": torch.empty(B, H, W, device=dev),
           "label": torch.empty(B, H, W, dtype=torch.int32, device=dev)}
    if rgb_in is not None:
        out["rgb"] = torch.empty(B, H, W, 3, device=dev)
    check(lib().ucsa_raster_draw(*args, _ptr(labels), _ptr(rgb_in), _ptr(ws), _ptr(pairs),
                                 n_pairs, pairs.numel(), _ptr(out["tri_id"]),
                                 _ptr(out["depth"]), _ptr(out["label"]), _ptr(out.get("rgb")),
                                 B * H * W, _stream()), "ucsa_raster_draw")
    return out


# ---------------------------------------------------------------------------
# label fusion (2D label maps voted onto mesh vertices)
# ---------------------------------------------------------------------------
def _vote_table(votes):
    """``votes`` [V, C+1] int64 (the bits of the uint64 table) -> V, C"""
    _gpu(votes, "votes", torch.int64, fixed=True)
    if votes.dim() != 2 or not (2 <= votes.shape[1] <= 256):
        raise _lib.UcsaError(f"votes must be [V, C+1] with 1 <= C <= 255, got "
                             f"{tuple(votes.shape)}")
    if votes.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("votes: V*(C+1) must be at most 2^31-1")
    return int(votes.shape[0]), int(votes.shape[1]) - 1


def _depth_gate(mesh_depth, sensor_depth, depth_tol, n, dev):
    """the optional depth gate of the two fusion ops -> mesh_depth, sensor_depth
    (float32, ``n`` elements each, or None) and the tolerance"""
    if (mesh_depth is None) != (sensor_depth is None):
        raise _lib.UcsaError("mesh_depth and sensor_depth come as a pair")
    if mesh_depth is None:
        if depth_tol is not None:
            raise _lib.UcsaError("depth_tol given without mesh_depth / sensor_depth")
        return None, None, 0.0
    if depth_tol is None:
        raise _lib.UcsaError("the depth gate needs depth_tol")
    tol = float(depth_tol)
    if not tol >= 0.0:
        raise _lib.UcsaError(f"depth_tol must be >= 0, got {depth_tol}")
    return (_gpu(mesh_depth, "mesh_depth", torch.float32, numel=n, device=dev),
            _gpu(sensor_depth, "sensor_depth", torch.float32, numel=n, device=dev), tol)


def fuse_label_votes(votes, vertex_id, pred, weight=None, mesh_depth=None, sensor_depth=None,
                     depth_tol=None, _one_atomic_per_pixel=False):
    """Pixels vote for (vertex, class) cells of ``votes`` [V, C+1] int64 (the
    bits of a uint64 table, zeroed by the caller; column 0 unused), in place;
    returns ``votes``.  ``vertex_id`` int32, any shape (the ``label`` of
    ``rasterize_mesh(..., vertex_labels=arange(1, V+1))``: 1-based, <= 0 = no
    vote), ``pred`` uint8 class ids (1..C vote), ``weight`` int32 in [0, 65535]
    or None (1 per vote), ``mesh_depth`` / ``sensor_depth`` fp32 z in scene
    units with ``depth_tol``: a pixel then votes only where sensor_depth > 0
    and |mesh_depth - sensor_depth| <= depth_tol.  All of vertex_id's size.
    Contract of ucsa_label_fuse_accumulate (include/ucsa_hip.h): integer sums,
    the same bytes whatever the order of pixels and calls."""
    V, Cn = _vote_table(votes)
    dev = votes.device
    vid = _gpu(vertex_id, "vertex_id", torch.int32, device=dev)
    n = vid.numel()
    pr = _gpu(pred, "pred", torch.uint8, numel=n, device=dev)
    if n > 0x7FFFFFFF:
        raise _lib.UcsaError("fuse_label_votes: at most 2^31-1 pixels per call")
    w = None if weight is None else _gpu(weight, "weight", torch.int32, numel=n, device=dev)
    md, sd, tol = _depth_gate(mesh_depth, sensor_depth, depth_tol, n, dev)
    row_width = int(vertex_id.shape[-1]) if vertex_id.dim() >= 2 else 0
    check(lib().ucsa_label_fuse_accumulate(
        _ptr(vid), _ptr(pr), _ptr(w), _ptr(md), _ptr(sd), tol, n, row_width, V, Cn,
        _ptr(votes), votes.numel(), 1 if _one_atomic_per_pixel else 0, _stream()),
        "ucsa_label_fuse_accumulate")
    return votes


def resolve_label_votes(votes, min_votes: int = 1):
    """``votes`` [V, C+1] -> dict of device tensors: ``label`` [V] int32 (the
    class with the largest sum, ties to the lower id, 0 where the row's total
    is below ``min_votes``), ``total`` and ``winner`` [V] int64 (the bits of
    uint64 sums; confidence = winner / total).  ucsa_label_fuse_resolve.  On a
    table filled by ``fuse_label_evidence`` the sums are evidence sums and
    ``min_votes`` is in evidence units (a confident view adds about 255)."""
    V, Cn = _vote_table(votes)
    min_votes = int(min_votes)
    if not 1 <= min_votes < 1 << 64:
        raise _lib.UcsaError(f"min_votes must be >= 1, got {min_votes}")
    dev = votes.device
    out = {"label": torch.empty(V, dtype=torch.int32, device=dev),
           "total": torch.empty(V, dtype=torch.int64, device=dev),
           "winner": torch.empty(V, dtype=torch.int64, device=dev)}
    check(lib().ucsa_label_fuse_resolve(_ptr(votes), V, Cn, min_votes, _ptr(out["label"]),
                                        _ptr(out["total"]), _ptr(out["winner"]), V,
                                        _stream()), "ucsa_label_fuse_resolve")
    return out


def log_evidence(x, from_logits: bool = False, floor_nats: float = 8.0):
    """Class beliefs ``x`` [B,C,H,W] (probabilities, or logits with
    ``from_logits``) -> evidence codes uint8 [B,H,W,C], pixel-major (the C
    codes of a pixel are C consecutive bytes, as ``accumulate_voxel_evidence``
    and ``fuse_label_evidence`` read them):
    e_c = 255 - rint(255 * min(-ln p_c, L) / L) with L = ``floor_nats``: p = 1
    gives 255, p <= e^-L gives 0.  A sum of codes over views is the clamped
    log-likelihood sum scaled by 255 / L; an all-zero row means "abstain" and
    cannot come out of a softmax over C <= 255 classes with L = 8.  Plain
    torch in fp32 on x's device (elementwise plumbing; the HIP is in the
    accumulation)."""
    if not (torch.is_tensor(x) and x.dim() == 4 and x.is_floating_point()):
        raise _lib.UcsaError("log_evidence: x must be a floating-point tensor [B,C,H,W]")
    if not 1 <= x.shape[1] <= 255:
        raise _lib.UcsaError(f"log_evidence: 1 <= C <= 255, got {x.shape[1]}")
    L = _positive(floor_nats, "log_evidence: floor_nats")
    x = x.float()
    nl = -(torch.log_softmax(x, dim=1) if from_logits else torch.log(x))
    nl = torch.nan_to_num(nl, nan=L, posinf=L, neginf=0.0).clamp_(0.0, L)
    e = 255.0 - torch.round(nl * 255.0 / L)
    return e.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def fuse_label_evidence(votes, vertex_id, scores, mesh_depth=None, sensor_depth=None,
                        depth_tol=None):
    """The soft form of ``fuse_label_votes``: pixels add their row of evidence
    codes to their vertex's row of ``votes`` [V, C+1] int64 (the same table;
    column 0 is left untouched), in place; returns ``votes``.  ``vertex_id``
    int32 [...] as for ``fuse_label_votes``, ``scores`` uint8 [..., C]
    (``log_evidence``; an all-zero row abstains), the optional depth gate as
    for ``fuse_label_votes``.  A pixel with 1 <= vertex_id <= V that passes the
    gate adds scores[pixel, c-1] to votes[vertex_id-1, c] for c = 1..C.
    ``resolve_label_votes`` reads the table as it is; its ``min_votes`` is then
    in evidence units.  Contract of ucsa_label_fuse_evidence
    (include/ucsa_hip.h): integer sums, the same bytes whatever the order of
    pixels and calls."""
    V, Cn = _vote_table(votes)
    dev = votes.device
    vid = _gpu(vertex_id, "vertex_id", torch.int32, device=dev)
    n = vid.numel()
    if n > 0x7FFFFFFF:
        raise _lib.UcsaError("fuse_label_evidence: at most 2^31-1 pixels per call")
    if not (torch.is_tensor(scores) and scores.dim() >= 1
            and tuple(scores.shape) == tuple(vertex_id.shape) + (Cn,)):
        raise _lib.UcsaError(f"scores must be uint8 {list(vertex_id.shape) + [Cn]} (vertex_id's "
                             "shape, then the table's C)")
    sc = _gpu(scores, "scores", torch.uint8, numel=n * Cn, device=dev)
    md, sd, tol = _depth_gate(mesh_depth, sensor_depth, depth_tol, n, dev)
    row_width = int(vertex_id.shape[-1]) if vertex_id.dim() >= 2 else 0
    check(lib().ucsa_label_fuse_evidence(
        _ptr(vid), _ptr(sc), _ptr(md), _ptr(sd), tol, n, row_width, V, Cn, _ptr(votes),
        votes.numel(), _stream()), "ucsa_label_fuse_evidence")
    return votes


def mesh_adjacency(faces, n_vertices: int):
    """The vertex adjacency of a triangle mesh as compressed rows, for
    ``smooth_label_table``: ``faces`` [F,3] int32 on the GPU -> (``offsets``
    int32 [V+1], ``neighbours`` int32 [E]); the neighbours of vertex v are
    ``neighbours[offsets[v]:offsets[v+1]]``, ascending.  Every undirected edge
    is stored once per direction, a face listed twice adds nothing, a
    degenerate face contributes only its proper edges (no self edges).  Plain
    torch on the device (sort and unique: plumbing, not a kernel)."""
    if not (torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int32
            and faces.dim() == 2 and faces.shape[1] == 3):
        raise _lib.UcsaError("faces must be an int32 [F,3] tensor on the GPU")
    V = int(n_vertices)
    if not 0 <= V <= 0x7FFFFFFF:
        raise _lib.UcsaError(f"n_vertices must be in 0..2^31-1, got {n_vertices}")
    f = faces.long()
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= V):
        raise _lib.UcsaError(f"faces index vertices outside 0..{V - 1}")
    a = torch.cat([f[:, 0], f[:, 1], f[:, 2]])
    b = torch.cat([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    key = torch.unique(torch.cat([a * V + b, b * V + a]))       # sorted: by vertex, then neighbour
    if key.numel() > 0x7FFFFFFF:
        raise _lib.UcsaError("mesh_adjacency: more than 2^31-1 directed edges")
    src = torch.div(key, max(V, 1), rounding_mode="floor")
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=faces.device)
    offsets[1:] = torch.cumsum(torch.bincount(src, minlength=V), 0)
    return offsets.to(torch.int32), (key - src * V).to(torch.int32)


def _adjacency(adjacency, device=None):
    """``mesh_adjacency``'s pair, two contiguous int32 vectors on ``device`` (None:
    the current one) -> offsets, neighbours"""
    try:
        offsets, neighbours = adjacency
    except (TypeError, ValueError):
        raise _lib.UcsaError("adjacency must be the (offsets, neighbours) pair of mesh_adjacency")
    offsets = _gpu(offsets, "adjacency: offsets", torch.int32, (None,), device=device, fixed=True)
    return offsets, _gpu(neighbours, "adjacency: neighbours", torch.int32, (None,),
                         device=offsets.device, fixed=True)


def smooth_label_table(votes, adjacency, iterations: int = 1, centre: int = 1):
    """Pool a mesh table over each vertex's neighbours -> a NEW table; ``votes``
    [V, C+1] int64 (the bits of the uint64 table of ``fuse_label_votes`` /
    ``fuse_label_evidence``) is not modified.  ``adjacency`` is
    ``mesh_adjacency``'s pair.  out[v, :] = centre * votes[v, :] + the sum of
    votes[n, :] over the neighbours n of v, in all C+1 columns, modulo 2^64; a
    vertex without neighbours gets centre * votes[v].  ``iterations`` = k gives
    the bytes of k single calls.  ``resolve_label_votes`` reads the result as
    it is; ``min_votes`` then counts pooled units.  Contract of
    ucsa_label_table_smooth (include/ucsa_hip.h)."""
    V, Cn = _vote_table(votes)
    offsets, neighbours = _adjacency(adjacency, votes.device)
    if offsets.numel() != V + 1:
        raise _lib.UcsaError(f"adjacency: offsets has {offsets.numel()} entries, the table has "
                             f"{V} vertices")
    centre = _centre(centre)
    _count(iterations, "iterations")
    src, spare = votes, None
    for _ in range(iterations):
        dst = torch.empty_like(votes) if spare is None else spare
        check(lib().ucsa_label_table_smooth(
            _ptr(src), _ptr(dst), V, Cn, _ptr(offsets), _ptr(neighbours), neighbours.numel(),
            centre, _stream()), "ucsa_label_table_smooth")
        spare = src if src is not votes else None
        src = dst
    return src


def mesh_components(adjacency):
    """Connected components of a mesh's vertex graph -> int32 [V]: the smallest
    vertex index of each vertex's component (an isolated vertex gets its own).
    ``adjacency`` is ``mesh_adjacency``'s (offsets, neighbours) pair; it is not
    modified.  Contract of ucsa_graph_components (include/ucsa_hip.h)."""
    offsets, neighbours = _adjacency(adjacency)
    if offsets.numel() < 1:
        raise _lib.UcsaError("adjacency: offsets has V + 1 entries, got none")
    V = offsets.numel() - 1
    labels = torch.empty(V, dtype=torch.int32, device=offsets.device)
    check(lib().ucsa_graph_components(_ptr(offsets), _ptr(neighbours), V, neighbours.numel(),
                                      _ptr(labels), _stream()), "ucsa_graph_components")
    return labels


# ---------------------------------------------------------------------------
# mesh simplification by vertex clustering
# ---------------------------------------------------------------------------
SIMPLIFY_MAX_DIM = 1 << 18
_NO_CLUSTER = 0x7FFFFFFFFFFFFFFF


def _vertex_attributes(normals, rgb, labels, n, dev):
    """the optional per-vertex inputs of simplify_mesh and sample_mesh_surface ->
    normals float32 [n,3], rgb uint8 [n,3], labels uint8 [n] (given as any integer
    type, read back to be in 0..255), each contiguous on ``dev`` or None"""
    nrm = None if normals is None else _gpu(normals, "normals", torch.float32, (n, 3), device=dev)
    col = None if rgb is None else _gpu(rgb, "rgb", torch.uint8, (n, 3), device=dev)
    lab = None
    if labels is not None:
        _gpu(labels, "labels", _INTEGER, (n,), device=dev)
        if n and (int(labels.min()) < 0 or int(labels.max()) > 255):
            raise _lib.UcsaError("labels must be in 0..255")
        lab = labels.to(torch.uint8).contiguous()
    return nrm, col, lab


def simplify_mesh(verts, faces, cell, normals=None, rgb=None, labels=None,
                  split_labels: bool = False, origin=None):
    """Simplify a triangle mesh by vertex clustering (Rossignac-Borrel): the
    vertices of one cell of a uniform grid of edge ``cell`` become one vertex.
    ``verts`` float32 [V,3] and ``faces`` int32 [F,3] on the GPU; per vertex and
    optional ``normals`` float32 [V,3], ``rgb`` uint8 [V,3], ``labels`` an
    integer tensor [V] with values 0..255 (0 = none).  A cluster is a cell; with
    ``split_labels`` it is a (cell, label) pair, so vertices of different
    classes in one cell are never merged and class borders keep their place.
    ``origin`` (3 floats) defaults to the minimum corner of the finite vertices;
    dims = floor(extent / cell) + 1 per axis, at most 2^18.  -> dict:
    ``verts`` float32 [K,3] (the members' mean, summed as offsets from the first
    member), ``count`` int32 [K] and, for the inputs given, ``normals`` (the
    normalised sum), ``rgb`` uint8 (the mean, half up), ``labels`` uint8 (the
    most frequent label > 0, ties to the smallest; 0 if none): one row per
    cluster, in ascending key order (x-major cell order, then label when
    split); ``faces`` int32 [F',3]: every face through the clusters of its
    corners, rotated to start at its smallest index, without the degenerate
    ones (two corners on one cluster, a corner outside [0, V) or on a
    non-finite vertex) and without repeated triples (the lowest input face is
    kept; a reversed copy is another triple and stays), in their former
    relative order; ``face_index`` int32 [F'] (the input face of each);
    ``vertex_map`` int32 [V] (the cluster of every input vertex, -1 for a
    non-finite one); ``origin``, ``cell``, ``dims``; ``degenerate`` and
    ``duplicate`` (how many faces went each way).  V = 0 and F = 0 are valid;
    the inputs are not modified.  One lane walks a cluster's members in order:
    a call that puts every vertex into one cell costs one lane walking all of
    them.  The keys, the per-cluster reduction and the face mapping are kernels
    (ucsa_vertex_cluster_keys, ucsa_cluster_reduce, ucsa_cluster_faces in
    include/ucsa_hip.h); the sort, the cluster boundaries, the de-duplication
    and the compaction are torch on the device."""
    pts, fc = _mesh(verts, faces)
    dev = pts.device
    n, nf = int(pts.shape[0]), int(fc.shape[0])
    nrm, col, lab = _vertex_attributes(normals, rgb, labels, n, dev)
    f32 = lambda v: float(torch.tensor(float(v), dtype=torch.float32))
    try:
        cell = f32(cell)
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"cell must be a number, got {cell!r}")
    _positive(cell, "cell (in float32)")
    lo, hi = _finite_box(pts, torch.isfinite(pts).all(1))
    if origin is not None:
        try:
            lo = [f32(v) for v in origin]
        except (TypeError, ValueError):
            raise _lib.UcsaError("origin must be three numbers")
        if len(lo) != 3 or not all(math.isfinite(v) for v in lo):
            raise _lib.UcsaError(f"origin must be three finite numbers, got {origin!r}")
    dims = tuple(int(math.floor(max(float(b) - float(a), 0.0) / cell)) + 1
                 for a, b in zip(lo, hi))
    if max(dims) > SIMPLIFY_MAX_DIM:
        raise _lib.UcsaError(f"cell {cell!r} needs {max(dims)} cells along an axis, more than "
                             f"2^18: raise cell")
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    check(lib().ucsa_vertex_cluster_keys(_ptr(pts), n, fvec(lo), cell, (C.c_uint32 * 3)(*dims),
                                         _ptr(lab), _ptr(keys), _stream()),
          "ucsa_vertex_cluster_keys")
    skeys, order64 = torch.sort(keys, stable=True)
    order = order64.to(torch.int32)
    n_fin = int((skeys != _NO_CLUSTER).sum()) if n else 0
    ident = skeys[:n_fin] if split_labels else skeys[:n_fin] >> 8
    _, inverse, counts = torch.unique_consecutive(ident, return_inverse=True, return_counts=True)
    K = int(counts.numel())
    first = torch.zeros(K + 1, dtype=torch.int32, device=dev)
    first[1:] = torch.cumsum(counts, 0)
    vertex_map = torch.full((n,), -1, dtype=torch.int32, device=dev)
    vertex_map[order64[:n_fin]] = inverse.to(torch.int32)
    out = {"verts": torch.empty((K, 3), dtype=torch.float32, device=dev),
           "count": torch.empty(K, dtype=torch.int32, device=dev)}
    if nrm is not None:
        out["normals"] = torch.empty((K, 3), dtype=torch.float32, device=dev)
    if col is not None:
        out["rgb"] = torch.empty((K, 3), dtype=torch.uint8, device=dev)
    if lab is not None:
        out["labels"] = torch.empty(K, dtype=torch.uint8, device=dev)
    check(lib().ucsa_cluster_reduce(_ptr(pts), _ptr(nrm), _ptr(col), _ptr(lab), n, _ptr(order),
                                    _ptr(first), K, _ptr(out["verts"]), _ptr(out.get("normals")),
                                    _ptr(out.get("rgb")), _ptr(out.get("labels")),
                                    _ptr(out["count"]), _stream()), "ucsa_cluster_reduce")
    tri = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    keep = torch.empty(nf, dtype=torch.uint8, device=dev)
    check(lib().ucsa_cluster_faces(_ptr(fc), nf, _ptr(vertex_map) if n else None, n, _ptr(tri),
                                   _ptr(keep), _stream()), "ucsa_cluster_faces")
    kept = torch.nonzero(keep).view(-1)
    n_kept = int(kept.numel())
    if n_kept:
        # equal triples, two columns at a time so that a key stays below 2^62
        t = tri[kept].long()
        ab = torch.unique(t[:, 0] * K + t[:, 1], return_inverse=True)[1]
        abc = torch.unique(ab * K + t[:, 2], return_inverse=True)[1]
        # a stable sort puts the lowest input face first in each group
        sg, pos = torch.sort(abc, stable=True)
        head = torch.ones_like(sg, dtype=torch.bool)
        head[1:] = sg[1:] != sg[:-1]
        face_index = kept[torch.sort(pos[head]).values]
    else:
        face_index = kept
    out["faces"] = tri[face_index].reshape(-1, 3)
    out["face_index"] = face_index.to(torch.int32)
    out["vertex_map"] = vertex_map
    out["origin"], out["cell"], out["dims"] = tuple(float(v) for v in lo), cell, dims
    out["degenerate"] = nf - n_kept
    out["duplicate"] = n_kept - int(face_index.numel())
    return out


# ---------------------------------------------------------------------------
# area-uniform sample points on a triangle mesh
# ---------------------------------------------------------------------------
SAMPLE_MAX_SAMPLES = 0x7FFFFFFF


def sample_mesh_surface(verts, faces, density, seed: int = 0, normals=None, rgb=None,
                        labels=None, max_samples: int = 1 << 26):
    """A deterministic, area-uniform, low-discrepancy point set on the surface of
    a triangle mesh, ``density`` points per unit area: the query points of 3D
    scores that weigh a surface by its area and not by its tessellation.
    ``verts`` float32 [V,3] and ``faces`` int32 [F,3] on the GPU; per vertex and
    optional ``normals`` float32 [V,3], ``rgb`` uint8 [V,3], ``labels`` an
    integer tensor [V] with values 0..255.  ``seed`` is a uint32.  -> dict:
    ``points`` float32 [S,3], ``face`` int32 [S] (ascending), ``bary`` float32
    [S,3] (multiples of 2^-24, non-negative, summing to exactly 1) and, for the
    inputs given, ``normals`` (the blend, normalised; zero where it vanishes),
    ``rgb`` uint8 (the blend, half up), ``labels`` uint8 (of the corner with the
    largest weight, the first on a tie, as ``transfer_labels`` decides); per
    face ``area`` float32 [F], ``count`` int32 [F] (area * density, rounded
    down after adding a hashed offset in [0, 1): no bias, so faces far smaller
    than 1 / density are sampled at the right rate) and ``first`` int32 [F+1]
    (the samples of face f are rows first[f] .. first[f+1]); ``n_samples`` = S
    and ``density`` (as rounded to float32).  A face with a corner index outside
    [0, V), a non-finite corner or a non-finite area has area 0 and no sample.
    A sample depends on (seed, face index, index inside the face) and the
    face's corners alone: a higher density keeps every earlier sample of a face
    and appends new ones, and editing one face moves no sample of another.
    More than ``max_samples`` (at most 2^31-1) samples is an error raised before
    anything of that size is allocated.  F = 0, V = 0 and S = 0 are valid; the
    inputs are not modified.  The counts and the samples are kernels
    (ucsa_face_sample_counts, ucsa_mesh_surface_samples in include/ucsa_hip.h);
    the prefix sum is torch on the device, in int64."""
    pts, fc = _mesh(verts, faces)
    dev = pts.device
    n, nf = int(pts.shape[0]), int(fc.shape[0])
    nrm, col, lab = _vertex_attributes(normals, rgb, labels, n, dev)
    try:
        density = float(torch.tensor(float(density), dtype=torch.float32))
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"density must be a number, got {density!r}")
    _positive(density, "density (in float32)")
    try:
        seed, max_samples = operator.index(seed), operator.index(max_samples)
    except TypeError:
        raise _lib.UcsaError("seed and max_samples must be integers")
    if not 0 <= seed <= 0xFFFFFFFF:
        raise _lib.UcsaError(f"seed must be in 0..2^32-1, got {seed!r}")
    if max_samples < 0:
        raise _lib.UcsaError(f"max_samples must not be negative, got {max_samples!r}")
    max_samples = min(max_samples, SAMPLE_MAX_SAMPLES)
    area = torch.empty(nf, dtype=torch.float32, device=dev)
    count = torch.empty(nf, dtype=torch.int32, device=dev)
    check(lib().ucsa_face_sample_counts(_ptr(pts) if n else None, n, _ptr(fc), nf, density, seed,
                                        _ptr(area), _ptr(count), _stream()),
          "ucsa_face_sample_counts")
    first64 = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    first64[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    S = int(first64[nf])
    if S > max_samples:
        raise _lib.UcsaError(f"density {density!r} gives {S} samples, more than max_samples = "
                             f"{max_samples}: lower density")
    first = first64.to(torch.int32)
    out = {"points": torch.empty((S, 3), dtype=torch.float32, device=dev),
           "face": torch.empty(S, dtype=torch.int32, device=dev),
           "bary": torch.empty((S, 3), dtype=torch.float32, device=dev)}
    if nrm is not None:
        out["normals"] = torch.empty((S, 3), dtype=torch.float32, device=dev)
    if col is not None:
        out["rgb"] = torch.empty((S, 3), dtype=torch.uint8, device=dev)
    if lab is not None:
        out["labels"] = torch.empty(S, dtype=torch.uint8, device=dev)
    check(lib().ucsa_mesh_surface_samples(_ptr(pts) if n else None, n, _ptr(fc), nf, _ptr(first), S,
                                          seed, _ptr(nrm), _ptr(col), _ptr(lab),
                                          _ptr(out["points"]), _ptr(out["face"]),
                                          _ptr(out["bary"]), _ptr(out.get("normals")),
                                          _ptr(out.get("rgb")), _ptr(out.get("labels")),
                                          _stream()), "ucsa_mesh_surface_samples")
    out.update(area=area, count=count, first=first, n_samples=S, density=density)
    return out
