"""The depth front end: a table-driven bilateral filter, the back-projected
point and a normal per pixel, and the mask that rejects depth edges and grazing
views.  Reached as ``ops.depth.filter_depth``, ``ops.depth.depth_normals`` and
``ops.depth.depth_frontend`` (both in one launch).  ``utils.depth_frontend``
sits on it."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from .._lib import check, lib
from ._args import _f32, _gpu, _non_negative, _positive, _ptr, _stream

RANGE_BINS = 256
MAX_RADIUS = 4
MEASURED, NORMAL, EDGE, GRAZING = 1, 2, 4, 8


def bilateral_tables(radius: int, sigma_space: float, Q: int = RANGE_BINS):
    """The two weight tables of the filter -> dict: ``radius``, ``w_space``
    [(2r+1)^2] and ``w_range`` [Q], numpy float32: exp in float64, rounded once.
    ``w_space[(dy+r)(2r+1) + (dx+r)] = exp(-(dx^2 + dy^2) / (2 sigma_space^2))``
    (pixels); ``w_range[q] = exp(-((q + 1/2) 3/Q)^2 / 2)``: the Gaussian of the
    depth difference at the middle of bin q, the bins covering three sigma."""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise _lib.UcsaError(f"radius must be an integer in 1..{MAX_RADIUS}, got {radius!r}")
    sigma_space = _positive(sigma_space, "sigma_space")
    if Q != RANGE_BINS:
        raise _lib.UcsaError(f"Q must be {RANGE_BINS}: the kernels' table length, got {Q!r}")
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = k[:, None] ** 2 + k[None, :] ** 2
    q = np.arange(Q, dtype=np.float64)
    return {"radius": radius,
            "w_space": np.exp(-d2 / (2.0 * sigma_space ** 2)).astype(np.float32).reshape(-1),
            "w_range": np.exp(-0.5 * ((q + 0.5) * 3.0 / Q) ** 2).astype(np.float32)}


def tables_on(tables, device):
    """``bilateral_tables``' dict with both tables as tensors on ``device``, so
    that a sequence of frames uploads them once"""
    out = dict(tables)
    for k in ("w_space", "w_range"):
        t = out[k]
        if not torch.is_tensor(t):
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(t, np.float32)))
        out[k] = t.to(device)
    return out


def _frames(depth):
    """``depth`` [B,H,W] on the GPU -> float32 contiguous, (B, H, W)"""
    if not torch.is_tensor(depth):
        raise _lib.UcsaError(f"depth must be a [B,H,W] tensor on the GPU: the HIP path has no CPU "
                             f"fallback; got {type(depth).__name__}")
    depth = _f32(depth, "depth")
    if depth.dim() != 3 or min(depth.shape) < 1 or max(depth.shape[1:]) > 16384:
        raise _lib.UcsaError(f"depth must be [B,H,W] with B >= 1 and 1 <= H, W <= 16384, got "
                             f"{tuple(depth.shape)}")
    return depth, tuple(int(s) for s in depth.shape)


def _tables(tables, dev):
    try:
        r, ws, wr = tables["radius"], tables["w_space"], tables["w_range"]
    except (TypeError, KeyError):
        raise _lib.UcsaError("tables must be the dict of ops.depth.bilateral_tables")
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= MAX_RADIUS:
        raise _lib.UcsaError(f"tables: radius must be an integer in 1..{MAX_RADIUS}, got {r!r}")
    if not (torch.is_tensor(ws) and torch.is_tensor(wr)):
        t = tables_on(tables, dev)
        ws, wr = t["w_space"], t["w_range"]
    ws = _gpu(ws, "tables: w_space", torch.float32, numel=(2 * r + 1) ** 2, device=dev)
    wr = _gpu(wr, "tables: w_range", torch.float32, numel=RANGE_BINS, device=dev)
    return r, ws, wr


def _range(depth_min, depth_max):
    depth_min, depth_max = float(depth_min), float(depth_max)
    if math.isnan(depth_min) or not depth_max >= depth_min:
        raise _lib.UcsaError(f"depth_min must not be NaN and depth_max >= depth_min, got "
                             f"{depth_min!r}, {depth_max!r}")
    return depth_min, depth_max


def _camera(intrinsics):
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    if not (fx > 0 and fy > 0 and all(math.isfinite(v) for v in (fx, fy, cx, cy))):
        raise _lib.UcsaError(f"intrinsics must have fx, fy > 0 and be finite, got "
                             f"{(fx, fy, cx, cy)}")
    return fx, fy, cx, cy


def _min_cos(min_cos):
    min_cos = float(min_cos)
    if not -1.0 <= min_cos <= 1.0:
        raise _lib.UcsaError(f"min_cos must be in [-1, 1], got {min_cos!r}")
    return min_cos


def filter_depth(depth, tables, sigma_depth: float, sigma_z2: float = 0.0,
                 depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """Bilateral filter of ``depth`` [B,H,W] (float32 z-depth on the GPU; 0, NaN,
    inf and anything outside [depth_min, depth_max] = no measurement) -> the
    filtered frames, float32 [B,H,W], 0 where the input has no measurement.
    ``tables``: ``bilateral_tables``' dict (or ``tables_on``'s).  A neighbour
    z_n of a centre z is weighted by the space table times the range table at
    |z_n - z| in units of 3 sigma / 256, sigma = ``sigma_depth`` +
    ``sigma_z2`` z^2, and takes no part beyond three sigma; the result is z plus
    the weighted mean difference.  ``depth`` is not modified.  Contract of
    ucsa_depth_filter (include/ucsa_hip.h)."""
    depth, (B, H, W) = _frames(depth)
    r, ws, wr = _tables(tables, depth.device)
    sigma_depth = _positive(sigma_depth, "sigma_depth")
    sigma_z2 = _non_negative(sigma_z2, "sigma_z2")
    depth_min, depth_max = _range(depth_min, depth_max)
    out = torch.empty_like(depth)
    check(lib().ucsa_depth_filter(_ptr(depth), B, H, W, _ptr(ws), r, _ptr(wr), sigma_depth,
                                  sigma_z2, depth_min, depth_max, _ptr(out), _stream()),
          "ucsa_depth_filter")
    return out


def depth_normals(depth, intrinsics, max_jump: float, max_jump_z2: float = 0.0,
                  min_cos: float = 0.0, depth_min: float = 1e-6, depth_max: float = 3.0e38):
    """Points, normals and the mask of ``depth`` [B,H,W] (float32 on the GPU,
    filtered or raw) -> dict: ``points`` [B,H,W,3] float32 in the camera frame
    (``utils.registration.backproject``'s expression), ``normals`` [B,H,W,3]
    unit, facing the camera, ``mask`` [B,H,W] uint8 of the bits MEASURED (1),
    NORMAL (2), EDGE (4: a measured 8-neighbour differs by more than
    ``max_jump`` + ``max_jump_z2`` z^2) and GRAZING (8: the cosine between the
    normal and the view ray is below ``min_cos``).  Zero rows where a pixel has
    no measurement or no normal.  ``intrinsics`` (fx, fy, cx, cy).  Contract of
    ucsa_depth_normals (include/ucsa_hip.h)."""
    depth, (B, H, W) = _frames(depth)
    fx, fy, cx, cy = _camera(intrinsics)
    max_jump = _non_negative(max_jump, "max_jump")
    max_jump_z2 = _non_negative(max_jump_z2, "max_jump_z2")
    min_cos = _min_cos(min_cos)
    depth_min, depth_max = _range(depth_min, depth_max)
    dev = depth.device
    points = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    check(lib().ucsa_depth_normals(_ptr(depth), B, H, W, fx, fy, cx, cy, max_jump, max_jump_z2,
                                   min_cos, depth_min, depth_max, _ptr(points), _ptr(normals),
                                   _ptr(mask), _stream()), "ucsa_depth_normals")
    return {"points": points, "normals": normals, "mask": mask}


def depth_frontend(depth, tables, intrinsics, sigma_depth: float, max_jump: float,
                   sigma_z2: float = 0.0, max_jump_z2: float = 0.0, min_cos: float = 0.0,
                   reject: int = EDGE | GRAZING, depth_min: float = 1e-6,
                   depth_max: float = 3.0e38):
    """``filter_depth`` and ``depth_normals`` of its result in one launch -> dict:
    ``depth`` (the filtered frames), ``points``, ``normals``, ``mask`` and
    ``clean``: the filtered frames with 0 wherever ``mask & reject``, ``reject``
    a set of EDGE | GRAZING: frames ``ops.integrate_tsdf`` and the vote kernels
    take.  The bytes are those of the two calls.  Contract of
    ucsa_depth_frontend (include/ucsa_hip.h)."""
    depth, (B, H, W) = _frames(depth)
    r, ws, wr = _tables(tables, depth.device)
    fx, fy, cx, cy = _camera(intrinsics)
    sigma_depth = _positive(sigma_depth, "sigma_depth")
    sigma_z2 = _non_negative(sigma_z2, "sigma_z2")
    max_jump = _non_negative(max_jump, "max_jump")
    max_jump_z2 = _non_negative(max_jump_z2, "max_jump_z2")
    min_cos = _min_cos(min_cos)
    if isinstance(reject, bool) or not isinstance(reject, int) or reject & ~(EDGE | GRAZING):
        raise _lib.UcsaError(f"reject must be a set of EDGE (4) | GRAZING (8), got {reject!r}")
    depth_min, depth_max = _range(depth_min, depth_max)
    dev = depth.device
    filtered, clean = torch.empty_like(depth), torch.empty_like(depth)
    points = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    check(lib().ucsa_depth_frontend(_ptr(depth), B, H, W, _ptr(ws), r, _ptr(wr), sigma_depth,
                                    sigma_z2, fx, fy, cx, cy, max_jump, max_jump_z2, min_cos,
                                    reject, depth_min, depth_max, _ptr(filtered), _ptr(clean),
                                    _ptr(points), _ptr(normals), _ptr(mask), _stream()),
          "ucsa_depth_frontend")
    return {"depth": filtered, "clean": clean, "points": points, "normals": normals,
            "mask": mask}
