"""The depth front end: a table-driven bilateral filter, the back-projected
point and a normal per pixel, and the mask that rejects depth edges and grazing
views.  Reached as ``ops.depth.filter_depth``, ``ops.depth.depth_normals`` and
``ops.depth.depth_frontend`` (both in one launch).  ``utils.depth_frontend``
sits on it.  ``ops.depth.depth_confidence`` turns those outputs into a weight
per pixel and ``ops.depth.integrate_tsdf_weighted`` integrates with it."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib
from .._lib import check, fvec, lib
from ._args import (_f32, _gpu, _non_negative, _positive, _ptr, _stream, _views,
                    volume_lattice)

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


def depth_confidence(points, normals, mask, sigma_depth: float, sigma_z2: float = 0.0,
                     cos_floor: float = 0.1, reject: int = EDGE | GRAZING):
    """The weight of every pixel's measurement for ``integrate_tsdf_weighted``,
    from ``depth_normals`` / ``depth_frontend``'s ``points`` [B,H,W,3],
    ``normals`` [B,H,W,3] and ``mask`` [B,H,W] uint8 -> float32 [B,H,W]: 0 where
    the pixel is not measured or carries a bit of ``reject``; elsewhere
    (``sigma_depth`` / (``sigma_depth`` + ``sigma_z2`` z^2))^2 -- the inverse
    variance of the front end's noise model relative to z = 0 -- times the
    cosine between normal and view ray, clamped to [``cos_floor``, 1]
    (``cos_floor`` where the pixel has no normal), so that no measured pixel is
    silenced.  Contract of ucsa_depth_confidence (include/ucsa_hip.h)."""
    if not (torch.is_tensor(points) and torch.is_tensor(normals) and torch.is_tensor(mask)):
        raise _lib.UcsaError("points, normals and mask must be tensors on the GPU: the HIP path "
                             "has no CPU fallback")
    points = _gpu(points, "points", torch.float32, (None, None, None, 3))
    B, H, W = (int(s) for s in points.shape[:3])
    if min(B, H, W) < 1 or max(H, W) > 16384:
        raise _lib.UcsaError(f"points must be [B,H,W,3] with B >= 1 and 1 <= H, W <= 16384, got "
                             f"{tuple(points.shape)}")
    dev = points.device
    normals = _gpu(normals, "normals", torch.float32, (B, H, W, 3), device=dev)
    mask = _gpu(mask, "mask", torch.uint8, (B, H, W), device=dev)
    sigma_depth = _positive(sigma_depth, "sigma_depth")
    sigma_z2 = _non_negative(sigma_z2, "sigma_z2")
    cos_floor = float(cos_floor)
    if not 0.0 < cos_floor <= 1.0:
        raise _lib.UcsaError(f"cos_floor must be in (0, 1], got {cos_floor!r}")
    if isinstance(reject, bool) or not isinstance(reject, int) or reject & ~(EDGE | GRAZING):
        raise _lib.UcsaError(f"reject must be a set of EDGE (4) | GRAZING (8), got {reject!r}")
    weight = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    check(lib().ucsa_depth_confidence(_ptr(points), _ptr(normals), _ptr(mask), B, H, W,
                                      sigma_depth, sigma_z2, cos_floor, reject, _ptr(weight),
                                      _stream()), "ucsa_depth_confidence")
    return weight


def integrate_tsdf_weighted(volume, depth, pixel_weight, poses, intrinsics, trunc: float,
                            color=None, max_weight: float = 65504.0, depth_min: float = 1e-6,
                            depth_max: float = 3.0e38):
    """``ops.integrate_tsdf`` with a weight per pixel: ``pixel_weight`` [B,H,W]
    float32 on the GPU (``depth_confidence``'s map, or any other); every other
    argument as there.  A pixel whose weight is not finite and > 0 takes no
    part; a measurement x enters as tsdf = (tsdf W + x w) / (W + w), W = min(W +
    w, ``max_weight``).  In place; returns ``volume``.  Weights of 1.0 give
    ``integrate_tsdf``'s bytes, and any split of the views over calls gives the
    same bytes.  The volume's ``weight`` is then in units of pixel weight -- a
    voxel seen once at w = 0.3 holds 0.3 -- and so is every ``min_weight`` that
    is compared with it.  Contract of ucsa_tsdf_integrate_weighted
    (include/ucsa_hip.h)."""
    (nx, ny, nz), dev = volume_lattice(volume)
    tsdf, weight, rgb = volume["tsdf"], volume["weight"], volume.get("rgb")
    depth, poses, (B, H, W), (fx, fy, cx, cy) = _views(depth, poses, intrinsics, dev)
    pixel_weight = _gpu(pixel_weight, "pixel_weight", torch.float32, (B, H, W), device=dev)
    if (color is None) != (rgb is None):
        raise _lib.UcsaError("color frames and a colour volume come as a pair")
    if color is not None:
        color = _gpu(color, "color", torch.uint8, (B, H, W, 3), device=dev)
    check(lib().ucsa_tsdf_integrate_weighted(
        _ptr(tsdf), _ptr(weight), _ptr(rgb), nx, ny, nz, fvec(volume["origin"]),
        fvec(volume["spacing"]), _ptr(depth), _ptr(pixel_weight), _ptr(color), _ptr(poses), B,
        fx, fy, cx, cy, H, W, float(trunc), float(max_weight), float(depth_min),
        float(depth_max), _stream()), "ucsa_tsdf_integrate_weighted")
    return volume


def pyramid_down(depth, max_jump: float, max_jump_z2: float = 0.0, depth_min: float = 1e-6,
                 depth_max: float = 3.0e38):
    """One level of the depth pyramid: ``depth`` [B,H,W] (float32 on the GPU) ->
    float32 [B,ceil(H/2),ceil(W/2)].  A coarse pixel takes its 2 x 2 block (what
    exists of it at an odd edge): with z0 the smallest measured depth of the
    block, the mean of the measured members within ``max_jump`` +
    ``max_jump_z2`` z0^2 of z0, as z0 plus the mean offset; 0 where nothing is
    measured.  The foreground wins, so a depth edge is not averaged across, and
    a constant block keeps its bits.  The coarse level's intrinsics are
    (fx/2, fy/2, cx/2, cy/2).  ``depth`` is not modified.  Contract of
    ucsa_depth_pyramid_down (include/ucsa_hip.h)."""
    depth, (B, H, W) = _frames(depth)
    max_jump = _non_negative(max_jump, "max_jump")
    max_jump_z2 = _non_negative(max_jump_z2, "max_jump_z2")
    depth_min, depth_max = _range(depth_min, depth_max)
    out = torch.empty((B, -(-H // 2), -(-W // 2)), dtype=torch.float32, device=depth.device)
    check(lib().ucsa_depth_pyramid_down(_ptr(depth), B, H, W, max_jump, max_jump_z2, depth_min,
                                        depth_max, _ptr(out), _stream()),
          "ucsa_depth_pyramid_down")
    return out
