"""The depth front end of the mapping chain, KinectFusion's first stage: a depth
frame is filtered (a bilateral filter whose range sigma may grow with z^2, as a
structured-light or time-of-flight sensor's noise does), back-projected, given a
normal per pixel, and the pixels on depth edges -- where sensors report "flying"
depths between the two surfaces -- or seen at a grazing angle are rejected
before the frame is integrated, voted with or tracked.

    depth --ops.depth.depth_frontend--> clean  --> ops.integrate_tsdf, the votes
                                        points --> registration (tracking)

``DepthFilter`` holds the settings; every consumer takes ``depth_filter=None``
and with None none of this is entered.  ``simulate_sensor_noise`` (numpy, no
GPU) makes the frames this is for out of exact ones: ``SyntheticRoom``'s depth
has no noise, no quantisation and no flying pixels.  ``ViewWeights`` (default
off as well: ``view_weights=None``) turns the same run's points, normals and
mask into a weight per pixel -- inverse variance under the filter's noise model
times the viewing cosine -- and the consumers then integrate ``clean`` through
``ops.depth.integrate_tsdf_weighted``.

Not here: hole filling, guidance by the colour image (the depth pyramid is
``ops.depth.pyramid_down``, used by ``utils.registration.frame_maps``)."""
from __future__ import annotations

import dataclasses

import numpy as np

EDGE, GRAZING = 4, 8


@dataclasses.dataclass(frozen=True)
class DepthFilter:
    """Settings of the front end.  ``radius`` (1..4 pixels) and ``sigma_space``
    (pixels) shape the window; a neighbour counts with a Gaussian of its depth
    difference over sigma = ``sigma_depth`` + ``sigma_z2`` z^2 (scene units) and
    not at all beyond three sigma.  A neighbour further than ``max_jump`` +
    ``max_jump_z2`` z^2 in depth is across a depth edge: it is kept out of the
    normal and marks the pixel as an edge pixel.  ``min_cos``: the least cosine
    between normal and view ray that is not grazing.  ``reject_edges`` /
    ``reject_grazing``: which of the two marks remove a pixel."""
    radius: int = 2
    sigma_space: float = 1.0
    sigma_depth: float = 0.01
    sigma_z2: float = 0.0
    max_jump: float = 0.05
    max_jump_z2: float = 0.0
    min_cos: float = 0.1
    reject_edges: bool = True
    reject_grazing: bool = True

    @property
    def reject(self) -> int:
        return (EDGE if self.reject_edges else 0) | (GRAZING if self.reject_grazing else 0)

    def scaled(self, unit: float) -> "DepthFilter":
        """the same filter for depths multiplied by ``unit`` (metres -> scene
        units): the lengths scale with it, the z^2 coefficients against it"""
        unit = float(unit)
        return dataclasses.replace(
            self, sigma_depth=self.sigma_depth * unit, max_jump=self.max_jump * unit,
            sigma_z2=self.sigma_z2 / unit, max_jump_z2=self.max_jump_z2 / unit)

    @classmethod
    def from_string(cls, spec: str) -> "DepthFilter":
        """``"radius=3,sigma_space=1.5,sigma_depth=0.02,reject_grazing=0"``: a
        comma-separated list of field=value over the defaults; ``"default"`` or
        an empty string gives the defaults."""
        fields = {f.name: f.type for f in dataclasses.fields(cls)}
        kw = {}
        spec = spec.strip()
        for item in ([] if spec in ("", "default") else spec.split(",")):
            name, sep, value = (s.strip() for s in item.partition("="))
            if not sep or name not in fields:
                raise ValueError(f"depth filter: {item!r} is not one of " +
                                 ", ".join(f"{n}=" for n in fields))
            kind = fields[name] if isinstance(fields[name], str) else fields[name].__name__
            if kind == "bool":
                if value.lower() not in ("0", "1", "false", "true"):
                    raise ValueError(f"depth filter: {name} takes 0 or 1, got {value!r}")
                kw[name] = value.lower() in ("1", "true")
            else:
                kw[name] = int(value) if kind == "int" else float(value)
        return cls(**kw)


@dataclasses.dataclass(frozen=True)
class ViewWeights:
    """Settings of the per-pixel weight of ``ops.depth.integrate_tsdf_weighted``
    (``frame_weights``): w = (sigma_depth / (sigma_depth + sigma_z2 z^2))^2 times
    the cosine between normal and view ray, the cosine clamped to
    [``cos_floor``, 1].  ``sigma_depth`` / ``sigma_z2``: None means the
    ``DepthFilter``'s own value, so that the weight is the inverse variance of
    the noise model the filter was given."""
    cos_floor: float = 0.1
    sigma_depth: float = None
    sigma_z2: float = None

    def resolved(self, flt: DepthFilter):
        """(sigma_depth, sigma_z2) with ``flt``'s values in place of None"""
        return (flt.sigma_depth if self.sigma_depth is None else float(self.sigma_depth),
                flt.sigma_z2 if self.sigma_z2 is None else float(self.sigma_z2))

    def scaled(self, unit: float) -> "ViewWeights":
        """the same weights for depths multiplied by ``unit``, as ``DepthFilter.scaled``"""
        unit = float(unit)
        return dataclasses.replace(
            self, sigma_depth=None if self.sigma_depth is None else self.sigma_depth * unit,
            sigma_z2=None if self.sigma_z2 is None else self.sigma_z2 / unit)

    def least(self, flt: DepthFilter, z_max: float) -> float:
        """The least weight a kept pixel at depth <= ``z_max`` can get: the
        ``min_weight`` that, with weights on, means "seen at least once" as 1
        does without them."""
        sd, s2 = self.resolved(flt)
        return float(self.cos_floor) * (sd / (sd + s2 * float(z_max) ** 2)) ** 2

    @classmethod
    def from_string(cls, spec: str) -> "ViewWeights":
        """``"cos_floor=0.2,sigma_z2=0.004"``: a comma-separated list of
        field=value over the defaults; ``"default"`` or an empty string gives the
        defaults."""
        names = [f.name for f in dataclasses.fields(cls)]
        kw = {}
        spec = spec.strip()
        for item in ([] if spec in ("", "default") else spec.split(",")):
            name, sep, value = (s.strip() for s in item.partition("="))
            if not sep or name not in names:
                raise ValueError(f"view weights: {item!r} is not one of " +
                                 ", ".join(f"{n}=" for n in names))
            kw[name] = float(value)
        return cls(**kw)


_tables_cache = {}


def _tables(flt: DepthFilter, device):
    """the filter's two tables on ``device``, made and uploaded once per setting"""
    import torch

    from .. import ops
    key = (flt.radius, float(flt.sigma_space), str(torch.device(device)))
    if key not in _tables_cache:
        _tables_cache[key] = ops.depth.tables_on(
            ops.depth.bilateral_tables(flt.radius, flt.sigma_space), device)
    return _tables_cache[key]


def fused_is_faster(B: int, radius: int) -> bool:
    """Whether the one launch beats ``filter_depth`` + ``depth_normals`` for B
    frames: it filters an 18 x 18 region per 16 x 16 tile, which costs a wave
    more than the 1.27 the areas suggest (324 pixels are six waves' worth, 256
    four), so it wins where the launches or the normals' reload weigh more than
    half a filter: single frames and small windows (profiles/depth_time.txt:
    480 x 640, r = 4, 0.030 against 0.046 ms at B = 1, 0.373 against 0.207 ms at
    B = 16; r = 2, 0.125 against 0.127 ms at B = 16).  The bytes are the same."""
    return int(B) <= 2 or int(radius) <= 2


def run_frontend(depth, intrinsics, flt: DepthFilter, depth_min=1e-6, depth_max=3.0e38):
    """The front end of ``depth`` [B,H,W] (a float32 tensor on the GPU) with the
    settings ``flt`` -> ``ops.depth.depth_frontend``'s dict, from that call or,
    where ``fused_is_faster`` says so, from the two launches it is defined by"""
    import torch

    from .. import ops
    tables = _tables(flt, depth.device)
    if fused_is_faster(depth.shape[0], flt.radius):
        return ops.depth.depth_frontend(
            depth, tables, intrinsics, flt.sigma_depth, flt.max_jump, sigma_z2=flt.sigma_z2,
            max_jump_z2=flt.max_jump_z2, min_cos=flt.min_cos, reject=flt.reject,
            depth_min=depth_min, depth_max=depth_max)
    f = ops.depth.filter_depth(depth, tables, flt.sigma_depth, flt.sigma_z2, depth_min, depth_max)
    out = ops.depth.depth_normals(f, intrinsics, flt.max_jump, flt.max_jump_z2, flt.min_cos,
                                  depth_min, depth_max)
    out["depth"] = f
    out["clean"] = torch.where((out["mask"] & flt.reject) != 0, torch.zeros_like(f), f)
    return out


def new_stats():
    """the counts ``clean_depth`` and ``frame_points`` add to"""
    return {"pixels": 0, "measured": 0, "edge": 0, "grazing": 0, "rejected": 0}


def _count(stats, mask, reject):
    if stats is None:
        return
    m = mask.reshape(-1)
    stats["pixels"] += int(m.numel())
    stats["measured"] += int((m & 1).ne(0).sum())
    stats["edge"] += int((m & EDGE).ne(0).sum())
    stats["grazing"] += int((m & GRAZING).ne(0).sum())
    stats["rejected"] += int((m & reject).ne(0).sum())


def stats_line(stats) -> str:
    """the scripts' one ``depth_filter:`` line: the share of the measured pixels
    that carry each bit, and the share ``reject`` removed"""
    n = max(1, stats["measured"])
    return (f"depth_filter: measured {stats['measured']} of {stats['pixels']} pixels; "
            f"edge (bit 4) {stats['edge'] / n:.4f}, grazing (bit 8) {stats['grazing'] / n:.4f}, "
            f"rejected {stats['rejected'] / n:.4f} of the measured")


def clean_depth(depth, intrinsics, flt: DepthFilter, depth_min=1e-6, depth_max=3.0e38,
                stats=None):
    """``depth`` [B,H,W] or [H,W] (a float32 tensor on the GPU) -> the filtered
    frames with 0 at every pixel ``flt`` rejects, same shape: what
    ``ops.integrate_tsdf`` and the vote kernels take in place of the raw frames.
    ``stats`` (``new_stats()``) gains the frame's counts, at the price of one
    read-back."""
    d = depth if depth.dim() == 3 else depth[None]
    out = run_frontend(d, intrinsics, flt, depth_min, depth_max)
    _count(stats, out["mask"], flt.reject)
    return out["clean"] if depth.dim() == 3 else out["clean"][0]


def frame_weights(frontend_outputs, flt: DepthFilter, vw: ViewWeights):
    """``run_frontend``'s dict -> the weight of every pixel's measurement,
    float32 [B,H,W] on the GPU (``ops.depth.depth_confidence``): 0 at the pixels
    ``flt`` rejects -- the zeros of ``clean`` -- and in (0, 1] at the others"""
    from .. import ops
    sd, s2 = vw.resolved(flt)
    return ops.depth.depth_confidence(frontend_outputs["points"], frontend_outputs["normals"],
                                      frontend_outputs["mask"], sd, s2, cos_floor=vw.cos_floor,
                                      reject=flt.reject)


def new_weight_stats():
    """the sums ``weighted_depth`` adds to"""
    return {"kept": 0, "weight_sum": 0.0}


def weight_stats_line(stats) -> str:
    """the scripts' one ``view_weights:`` line: the mean weight of the kept pixels"""
    return (f"view_weights: mean weight {stats['weight_sum'] / max(1, stats['kept']):.4f} over "
            f"{stats['kept']} kept pixels")


def weighted_depth(depth, intrinsics, flt: DepthFilter, vw: ViewWeights, depth_min=1e-6,
                   depth_max=3.0e38, stats=None, weight_stats=None):
    """``depth`` [B,H,W] (a float32 tensor on the GPU) -> (``clean``, ``weight``),
    [B,H,W] each: ``clean_depth``'s frames and ``frame_weights`` of the same run
    of the front end, what ``ops.depth.integrate_tsdf_weighted`` takes.
    ``weight_stats`` (``new_weight_stats()``) gains the number of kept pixels and
    the sum of their weights, at the price of one read-back."""
    import torch
    out = run_frontend(depth, intrinsics, flt, depth_min, depth_max)
    _count(stats, out["mask"], flt.reject)
    w = frame_weights(out, flt, vw)
    if weight_stats is not None:
        weight_stats["kept"] += int((w > 0).sum())
        weight_stats["weight_sum"] += float(w.sum(dtype=torch.float64))
    return out["clean"], w


def frame_points(depth, intrinsics, flt: DepthFilter, stride: int = 1, depth_min=1e-6,
                 depth_max=3.0e38, stats=None):
    """One frame ``depth`` [H,W] (a tensor on the GPU) -> (``points`` [N,3],
    ``normals`` [N,3]) float32 in the camera frame: the filtered depth's points
    at every ``stride``-th row and column that is measured and not rejected, in
    row-major pixel order -- ``utils.registration.backproject``'s points of the
    kept pixels -- with their normals (zero rows where a kept pixel has none)."""
    out = run_frontend(depth[None].float(), intrinsics, flt, depth_min, depth_max)
    _count(stats, out["mask"], flt.reject)
    s = int(stride)
    mask = out["mask"][0, ::s, ::s]
    keep = ((mask & 1) != 0) & ((mask & flt.reject) == 0)
    return out["points"][0, ::s, ::s][keep].contiguous(), \
        out["normals"][0, ::s, ::s][keep].contiguous()


# ---------------------------------------------------------------------------
# a sensor model for exact depth frames (numpy, no GPU)
# ---------------------------------------------------------------------------
def _window_min_max(z, valid):
    """min and max of the valid depths in every pixel's 3x3 neighbourhood"""
    H, W = z.shape[-2:]
    lo = np.where(valid, z, np.inf)
    hi = np.where(valid, z, -np.inf)
    pad = [(0, 0)] * (z.ndim - 2) + [(1, 1), (1, 1)]
    lo_p = np.pad(lo, pad, constant_values=np.inf)
    hi_p = np.pad(hi, pad, constant_values=-np.inf)
    mn, mx = lo.copy(), hi.copy()
    for dy in range(3):
        for dx in range(3):
            mn = np.minimum(mn, lo_p[..., dy:dy + H, dx:dx + W])
            mx = np.maximum(mx, hi_p[..., dy:dy + H, dx:dx + W])
    return mn, mx


def simulate_sensor_noise(depth, seed: int = 0, sigma0: float = 0.0, sigma_z2: float = 0.0,
                          quantum: float = 0.0, flying_share: float = 0.0, jump: float = 0.1,
                          return_flying: bool = False):
    """What a depth sensor makes of the exact frames ``depth`` [..., H, W] (z-depth,
    0 or non-finite = none) -> float32 of the same shape, or with
    ``return_flying`` (frames, the bool mask of the flying pixels).  In this
    order: a pixel whose 3x3 neighbourhood's valid depths span more than
    ``jump`` becomes, with probability ``flying_share``, a flying pixel: a
    uniform mixture of that neighbourhood's minimum and maximum; every valid
    pixel gains Gaussian noise of sigma = ``sigma0`` + ``sigma_z2`` z^2; the
    result is rounded to multiples of ``quantum`` (0: not rounded).  Pixels
    without a measurement stay 0.  Deterministic for a ``seed``."""
    z = np.asarray(depth, np.float64)
    valid = np.isfinite(z) & (z > 0)
    z = np.where(valid, z, 0.0)
    rng = np.random.default_rng(int(seed))
    mn, mx = _window_min_max(z, valid)
    with np.errstate(invalid="ignore"):
        on_edge = valid & (mx - mn > float(jump))
    flying = on_edge & (rng.random(z.shape) < float(flying_share))
    mix = rng.random(z.shape)
    z = np.where(flying, np.where(flying, mn, 0.0) + mix * np.where(flying, mx - mn, 0.0), z)
    z = z + rng.standard_normal(z.shape) * (float(sigma0) + float(sigma_z2) * z * z)
    if quantum > 0:
        z = np.round(z / float(quantum)) * float(quantum)
    out = np.where(valid, np.maximum(z, 0.0), 0.0).astype(np.float32)
    return (out, flying) if return_flying else out
