"""Rays against a triangle mesh: the nearest hit and the any-hit form, over the
grid of ``ops.triangle_grid``.  Reached as ``ops.raycast.raycast_mesh`` and
``ops.raycast.mesh_occluded``."""
from __future__ import annotations

import ctypes as C
import math

import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import _gpu, _points3, _ptr, _stream


def _t_range(t, name: str, n: int, device):
    """a range end: a scalar -> (None, float); float32 [n] on ``device`` -> (tensor, 0.0)"""
    if torch.is_tensor(t):
        return _gpu(t, name, torch.float32, (n,), device=device), 0.0
    try:
        return None, float(t)
    except (TypeError, ValueError):
        raise _lib.UcsaError(f"{name} must be a number or a float32 [{n}] tensor on the GPU, got "
                             f"{type(t).__name__}")


def _entry_order(o, d, tmin_t, tmin, origin, org, cell, dm, dims):
    """The rays by the cell of their entry point: the point at t_min, or where the
    ray enters the grid's box if that comes later (elementwise torch; it orders
    the lanes and changes no result)."""
    lo = torch.tensor([float(v) for v in origin], dtype=torch.float32, device=o.device)
    hi = lo + torch.tensor([float(n) * cell for n in dims], dtype=torch.float32, device=o.device)
    inv = 1.0 / torch.where(d == 0, torch.full_like(d, 1e-30), d)
    t_in = torch.minimum((lo - o) * inv, (hi - o) * inv).max(dim=1).values
    start = tmin_t if tmin_t is not None else torch.full_like(t_in, max(tmin, -3.0e38))
    t0 = torch.nan_to_num(torch.maximum(t_in, start), nan=0.0, posinf=0.0, neginf=0.0)
    p = torch.nan_to_num(o + t0[:, None] * d, nan=0.0, posinf=3.0e38, neginf=-3.0e38).contiguous()
    n = int(p.shape[0])
    keys = torch.empty(n, dtype=torch.int32, device=o.device)
    check(lib().ucsa_point_cell_keys(_ptr(p), n, org, cell, dm, 1, _ptr(keys), _stream()),
          "ucsa_point_cell_keys")
    return torch.sort(keys, stable=True).indices.to(torch.int32)


def _ray_args(grid, origins, dirs, t_min, t_max, sort_rays: bool):
    o = _points3(origins, "origins")
    d = _points3(dirs, "dirs")
    n = int(o.shape[0])
    if d.device != o.device or int(d.shape[0]) != n:
        raise _lib.UcsaError(f"origins and dirs must be [N,3] on one device, got "
                             f"{tuple(o.shape)} on {o.device} and {tuple(d.shape)} on {d.device}")
    try:
        rec, offsets = grid["records"], grid["offsets"]
        origin, cell, dims, P = grid["origin"], float(grid["cell"]), grid["dims"], \
            int(grid["n_pairs"])
    except (TypeError, KeyError):
        raise _lib.UcsaError("grid must be the dict of ops.triangle_grid")
    ncells = int(dims[0]) * int(dims[1]) * int(dims[2])
    _gpu(rec, "grid: records", torch.float32, (P, 12), device=o.device, fixed=True)
    _gpu(offsets, "grid: offsets", torch.int32, numel=ncells + 1, device=o.device, fixed=True)
    tmin_t, tmin = _t_range(t_min, "t_min", n, o.device)
    tmax_t, tmax = _t_range(t_max, "t_max", n, o.device)
    org, dm = fvec(origin), (C.c_uint32 * 3)(*[int(x) for x in dims])
    order = None
    if sort_rays and n and P:
        order = _entry_order(o, d, tmin_t, tmin, origin, org, cell, dm, dims) if not math.isnan(tmin) \
            else None
    keep = (o, d, tmin_t, tmax_t, order)          # alive until the launch is enqueued
    args = (_ptr(rec) if P else None, _ptr(offsets) if P else None, P, org, cell, dm, _ptr(o),
            _ptr(d), _ptr(tmin_t), _ptr(tmax_t), tmin, tmax, _ptr(order), n)
    return args, n, o.device, keep


def raycast_mesh(grid, origins, dirs, t_min=0.0, t_max=math.inf, sort_rays: bool = False):
    """For each ray ``origins[i] + t * dirs[i]`` ([N,3] float32 on the GPU, the
    directions of any length) the first face of ``grid`` (``triangle_grid``'s
    dict) it hits with ``t_min <= t <= t_max`` -> (``face`` int32 [N], ``t``
    float32 [N], ``bary`` float32 [N,3]) on the device: the face, the ray
    parameter (a distance only for unit directions) and the hit point's
    barycentric weights of the face's three corners; -1, +inf and a zero row on
    a miss.  ``t_min`` / ``t_max`` are numbers or float32 [N] tensors; ``t_max``
    may be +inf and ``t_min`` -inf.  Among hits at the same ``t`` the smallest
    face index wins; both sides of a face are hit; a ray through a shared edge
    or vertex hits one of the faces that share it (the edge tests are exact);
    a non-finite ray or a zero direction hits nothing.  ``sort_rays`` hands the
    rays to the kernel by the cell of their entry point, so that a wave's lanes
    walk neighbouring cells; it changes time only.  The result does not depend
    on the grid's cell.  Contract of ucsa_raycast_mesh (include/ucsa_hip.h)."""
    args, n, dev, keep = _ray_args(grid, origins, dirs, t_min, t_max, sort_rays)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    t = torch.empty(n, dtype=torch.float32, device=dev)
    bary = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(lib().ucsa_raycast_mesh(*args, _ptr(face), _ptr(t), _ptr(bary), _stream()),
          "ucsa_raycast_mesh")
    return face, t, bary


def mesh_occluded(grid, origins, dirs, t_min=0.0, t_max=math.inf, sort_rays: bool = False):
    """Whether any face of ``grid`` is hit by each ray within ``[t_min, t_max]``
    -> uint8 [N] on the device: ``raycast_mesh(...)[0] >= 0`` without the search
    for the nearest hit (the walk ends at its first hit).  With ``dirs = P - C``
    and ``t_max`` a little below 1 it answers "is P visible from C".  Arguments
    as for ``raycast_mesh``.  Contract of ucsa_mesh_occluded (include/ucsa_hip.h)."""
    args, n, dev, keep = _ray_args(grid, origins, dirs, t_min, t_max, sort_rays)
    occluded = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib().ucsa_mesh_occluded(*args, _ptr(occluded), _stream()), "ucsa_mesh_occluded")
    return occluded
