"""What the wrappers share: pointers, torch's current stream, the grow-only
scratch buffers and the argument checks.  Every kernel is enqueued on the
CURRENT device's current stream, so every tensor handed to the library is
checked here, once, to live on that device (or on the device of the op's
primary tensor, which was checked that way)."""
from __future__ import annotations

import ctypes as C
import math
import threading
from typing import Optional

import torch

from .. import _lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_current_stream() -> int:
    if _raw_stream is not None:
        return int(_raw_stream(torch.cuda.current_device()))
    return int(torch.cuda.current_stream().cuda_stream)


def _stream():
    # torch's current stream on the current device; the raw getter is ~20x
    # cheaper than torch.cuda.current_stream() (a training step makes ~17 calls)
    return C.c_void_p(_raw_current_stream())


# ---------------------------------------------------------------------------
# scratch buffers
# ---------------------------------------------------------------------------
_march_ws = {}
_named_ws = {}


def _scratch_named(name: str, nbytes: int, device) -> torch.Tensor:
    """A grow-only scratch buffer of its own (not shared with _scratch's).
    Keyed by the calling THREAD as well as device and stream: the
    multi-launch ops (BatchNorm: stats -> finalize -> apply; augmentation: grey
    sums -> apply) pass intermediates through it, ctypes releases the GIL, and the
    trainer's prefetch thread issues on the same stream as the training step -- two
    threads sharing one buffer would overwrite each other's partial sums."""
    key = (name, device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    buf = _named_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _named_ws[key] = buf
    return buf


def _scratch(nbytes: int, device) -> torch.Tensor:
    key = (device, torch.cuda.current_stream().cuda_stream, threading.get_ident())
    buf = _march_ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8,
                          device=device)
        _march_ws[key] = buf
    return buf


# ---------------------------------------------------------------------------
# tensors
# ---------------------------------------------------------------------------
def _on_current_device(dev, what: str):
    cur = torch.cuda.current_device()
    if dev.index != cur:
        # kernels are enqueued on the CURRENT device's current stream
        raise _lib.UcsaError(f"{what} is on {dev} but the current device is cuda:{cur}: "
                             "call torch.cuda.set_device first")


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """``t`` on the current device -> float32 and contiguous (converted if need be)"""
    if not t.is_cuda:
        raise _lib.UcsaError(
            f"{name} must live on the GPU: the HIP path has no CPU fallback")
    _on_current_device(t.device, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


_INTEGER = "any integer type"      # a dtype of _gpu (bool is not one)


def _gpu(t, name: str, dtype=None, shape=None, numel=None, device=None, fixed: bool = False):
    """``t`` as a kernel may read it -> ``t.contiguous()``.  It must be a tensor on
    the GPU: on ``device``, the device of the op's primary tensor, or without one
    on the current device; of ``dtype`` (one, a tuple, or _INTEGER), never
    converted; of ``shape`` (None = any size) or of ``numel`` elements.  ``fixed``:
    the tensor is written in place or kept by the caller, so it must be contiguous
    as it stands."""
    ok = torch.is_tensor(t) and t.is_cuda
    if ok and device is None:
        _on_current_device(t.device, name)
    if ok and dtype is not None:
        ok = (not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)
              if dtype is _INTEGER else
              t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype)
    ok = (ok and (device is None or t.device == device)
          and (shape is None or (t.dim() == len(shape) and all(
              w is None or w == g for w, g in zip(shape, t.shape))))
          and (numel is None or t.numel() == numel) and (not fixed or t.is_contiguous()))
    if not ok:
        want = ", ".join(str(w) for w in (
            "contiguous" if fixed else None, dtype,
            None if shape is None else
            "[" + ",".join("*" if w is None else str(w) for w in shape) + "]",
            None if numel is None else f"{numel} elements",
            None if device is None else f"on {device}") if w is not None)
        got = (f"{t.dtype} {list(t.shape)} on {t.device}" if torch.is_tensor(t)
               else type(t).__name__)
        raise _lib.UcsaError(f"{name} must be a GPU tensor{want and ' (' + want + ')'}: the HIP "
                             f"path has no CPU fallback; got {got}")
    return t if fixed else t.contiguous()


def _i32(t: torch.Tensor, name: str) -> torch.Tensor:
    return _gpu(t, name, torch.int32, fixed=True)


def _inplace_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    """a tensor the kernel updates in place"""
    return _gpu(t, name, torch.float32, fixed=True)


def _points3(t, name: str):
    """[N,3] on the current device -> float32, contiguous"""
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and t.shape[1] == 3):
        raise _lib.UcsaError(f"{name} must be an [N,3] tensor on the GPU: the HIP path has no "
                             "CPU fallback")
    if t.shape[0] > 0x7FFFFFFF:
        raise _lib.UcsaError(f"{name} must have at most 2^31-1 rows")
    return _f32(t, name)


# ---------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------
def _positive(x, name: str) -> float:
    x = float(x)
    if not (x > 0 and math.isfinite(x)):
        raise _lib.UcsaError(f"{name} must be > 0 and finite, got {x!r}")
    return x


def _non_negative(x, name: str) -> float:
    x = float(x)
    if not (x >= 0 and math.isfinite(x)):
        raise _lib.UcsaError(f"{name} must be >= 0 and finite, got {x!r}")
    return x


def _count(x, name: str, least: int = 1) -> int:
    """a Python int (not a bool) >= ``least``"""
    if isinstance(x, bool) or not isinstance(x, int) or x < least:
        raise _lib.UcsaError(f"{name} must be an integer >= {least}, got {x!r}")
    return x


def _origin_spacing(what: str, origin, spacing):
    """a lattice's frame -> (origin, spacing), three floats each: finite, the
    spacing > 0 (one number stands for all three)"""
    spacing = [float(spacing)] * 3 if isinstance(spacing, (int, float)) else \
        [float(v) for v in spacing]
    origin = [float(v) for v in origin]
    if len(origin) != 3 or len(spacing) != 3:
        raise _lib.UcsaError(f"{what}: origin and spacing have 3 entries each")
    if not all(v > 0 and math.isfinite(v) for v in spacing):
        raise _lib.UcsaError(f"{what}: spacing must be > 0 and finite, got {spacing}")
    if not all(math.isfinite(v) for v in origin):
        raise _lib.UcsaError(f"{what}: origin must be finite, got {origin}")
    return origin, spacing


def _centre(centre) -> int:
    if _count(centre, "centre") > 255:
        raise _lib.UcsaError(f"centre must be an integer in 1..255, got {centre!r}")
    return centre


# ---------------------------------------------------------------------------
# cameras and views
# ---------------------------------------------------------------------------
def _cameras(poses, intrinsics, device, B: Optional[int] = None):
    """``poses`` [B,4,4] camera-to-world on ``device`` (``B`` views when given, at
    least one otherwise) and ``intrinsics`` (fx, fy, cx, cy) as for get_rays ->
    poses (float32, contiguous), B, (fx, fy, cx, cy)"""
    poses = _f32(poses, "poses")
    if (poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.device != device
            or (poses.shape[0] < 1 if B is None else poses.shape[0] != B)):
        raise _lib.UcsaError(f"poses must be [{'B' if B is None else B},4,4] on {device}, got "
                             f"{tuple(poses.shape)} on {poses.device}")
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    if not (fx > 0 and fy > 0 and all(math.isfinite(v) for v in (fx, fy, cx, cy))):
        raise _lib.UcsaError(f"intrinsics must have fx, fy > 0 and be finite, got "
                             f"{(fx, fy, cx, cy)}")
    return poses, int(poses.shape[0]), (fx, fy, cx, cy)


def _views(depth, poses, intrinsics, device):
    """B posed depth views on ``device``: ``depth`` [B,H,W], ``poses`` [B,4,4] ->
    depth, poses (float32, contiguous), (B, H, W), (fx, fy, cx, cy)"""
    depth = _f32(depth, "depth")
    if depth.dim() != 3 or depth.device != device:
        raise _lib.UcsaError(f"depth must be [B,H,W] on {device}, got {tuple(depth.shape)} on "
                             f"{depth.device}")
    B, H, W = (int(s) for s in depth.shape)
    poses, _, K = _cameras(poses, intrinsics, device, B)
    return depth, poses, (B, H, W), K


# ---------------------------------------------------------------------------
# volumes and their class tables
# ---------------------------------------------------------------------------
def volume_lattice(volume):
    """(nx, ny, nz), device of a ``tsdf_volume``, checked as every op that takes
    one needs it: ``tsdf`` and ``weight`` (and ``rgb`` [nx,ny,nz,3], if any)
    contiguous float32 [nx,ny,nz] on the current device."""
    tsdf = _inplace_f32(volume["tsdf"], "volume['tsdf']")
    if tsdf.dim() != 3:
        raise _lib.UcsaError("volume: tsdf and weight must be [nx,ny,nz] on one device")
    dev = tsdf.device
    _gpu(volume["weight"], "volume['weight']", torch.float32, tuple(tsdf.shape), device=dev,
         fixed=True)
    if volume.get("rgb") is not None:
        _gpu(volume["rgb"], "volume['rgb']", torch.float32, tuple(tsdf.shape) + (3,),
             device=dev, fixed=True)
    return tuple(int(s) for s in tsdf.shape), dev


def _class_planes(table, noun: str, dtype, lattice=None, device=None) -> int:
    """a class-major table [C+1,nx,ny,nz] of ``dtype`` (over ``lattice`` on
    ``device``, when given) -> C"""
    _gpu(table, noun, dtype, (None,) * 4 if lattice is None else (None,) + tuple(lattice),
         device=device, fixed=True)
    if not 2 <= table.shape[0] <= 256:
        raise _lib.UcsaError(f"{noun} must be [C+1,nx,ny,nz] with 1 <= C <= 255, got "
                             f"{tuple(table.shape)}")
    return int(table.shape[0]) - 1


# ---------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------
def _mesh(verts, faces, max_faces: int = 0x7FFFFFFF, any_integer: bool = False):
    """``verts`` [V,3] on the current device and ``faces`` [F,3] on the same, at
    most ``max_faces`` rows -> (verts float32, faces int32), contiguous.  ``faces``
    must be int32; with ``any_integer`` it may be of any integer type, its index
    range is read back and must lie in [0, V), and it is converted."""
    v = _points3(verts, "verts")
    f = _gpu(faces, "faces", _INTEGER if any_integer else torch.int32, (None, 3), device=v.device)
    V, F = int(v.shape[0]), int(f.shape[0])
    if F > max_faces:
        raise _lib.UcsaError(f"faces must have at most {max_faces} rows")
    if any_integer:
        lo_hi = torch.stack(torch.aminmax(f)).tolist() if F else [0, 0]
        if F and (lo_hi[0] < 0 or lo_hi[1] >= V):
            raise _lib.UcsaError(f"faces index outside [0, {V})")
        f = f.to(torch.int32)
    return v, f


def _finite_box(pts, ok):
    """the bounding box of the rows of ``pts`` [N,3] that ``ok`` marks (the finite
    ones) -> (lo, hi), three Python floats each; zeros when there is none"""
    if pts.shape[0] and bool(ok.any()):
        good = pts[ok]
        return good.min(0).values.tolist(), good.max(0).values.tolist()
    return [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
