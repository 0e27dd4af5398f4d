"""numpy restatement of the density pass (include/ucsa_hip.h:
``ucsa_sigma_mlp_fwd*``, ``ucsa_sigma_mlp_fwd_scatter``, ``ucsa_density_sorted``):
the sigma net 32 -> 64 (ReLU) -> 16 and ``sigma = exp(h[:, 0])``, alone and
behind the hash-grid encode.  The float64 yardstick of
tests/test_density_reference_cpu.py and tests/test_gpu_density_reference.py
(test infrastructure: plain numpy, no torch op, no GPU, no HIP library).

Nothing is restated here: the net, its running error bound and the sigma
interval are ``shade_numpy.sigma_forward(outputs=True)`` (the ``Mode`` units,
``_lin``, ``_q``, ``_relu_e``), positions / cells / features and their bound are
``hashgrid_numpy`` (``ray_points``, ``encode``, ``bound_fwd``).  This module adds
the end-to-end reference ``density_rays``, the comparison ``compare_density``,
the case builders both test files share and the deliberate mistakes of the
sharpness table.

Layout: a feature array is level-major ``feat [16, M, 2]``; the net's input row
is ``x[m, 2 level + c] = feat[level, m, c]`` (``to_rows`` / ``to_feat``).
"""
from types import SimpleNamespace as NS

import numpy as np

from tests import hashgrid_numpy as hn
from tests import shade_numpy as sn
from tests.shade_numpy import F32, F64

MODES = {"fp32": sn.FP32, "f16": sn.F16M(1.0), "x3": sn.X3, "h2": sn.H2}

SIZES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 2049)
WRAP_P = 4096
WRAP_M = {"fp32": 2048 * 256 + 17, "f16": 2048 * 512 + 17, "x3": 4096 * 256 + 17,
          "h2": 4096 * 256 + 17}
EXP_TARGETS = (-110.0, -104.0, -95.0, -87.4, -20.0, 0.0, 20.0, 88.0, 88.72 - 1e-3,
               88.72 + 1e-3, 89.0, 200.0)
FUSED_DEPTH = ((8, 8, 1), (8, 8, 16), (8, 8, 17), (9, 17, 5), (17, 23, 33), (8, 16, 256),
               (8, 8, 300), (8, 8, 1024))
FUSED_INDEX = ((9, 16, 70), (8, 8, 256))
MUTANTS = ("cols_c_major", "w2_rows_swapped", "sigma_from_h1", "sigma_clamped",
           "relu_dropped", "f16_hidden_unrounded", "tail_block_last_row", "scatter_to_m",
           "fused_level_12_for_8", "fused_no_tile_base", "fused_table_row_late")


def to_rows(feat):
    """feat [16, M, 2] -> x [M, 32]"""
    feat = np.asarray(feat)
    return np.ascontiguousarray(feat.transpose(1, 0, 2).reshape(feat.shape[1], 32))


def to_feat(x):
    """x [M, 32] -> feat [16, M, 2]"""
    x = np.asarray(x)
    return np.ascontiguousarray(x.reshape(x.shape[0], 16, 2).transpose(1, 0, 2))


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def density_rows(x, sigma_params, mode, e_x=None):
    """x [M, 32] (fp32 inputs; float64 with their bound ``e_x`` behind an encode)
    -> h, e_h, sigma_lo, sigma_hi (and every intermediate) in ``mode``."""
    mode = MODES[mode] if isinstance(mode, str) else mode
    return sn.sigma_forward(x, sigma_params, mode, e_feat=e_x, outputs=True)


def density_rays(levels, bound, table, rays_o, rays_d, z, aabb, sigma_params, mode):
    """``ucsa_density_sorted`` (and the staged pair it replaces) end to end,
    ray-major: p = clamp(o + d z), the 16 levels' trilinear features with their
    gather bound, the sigma net, the sigma interval.  Row r T + s belongs to
    sample s of ray r whatever order the kernel walks the samples in."""
    pts = hn.ray_points(rays_o, rays_d, z, aabb)
    feat, mag = hn.encode(levels, bound, pts, table)
    ref = density_rows(to_rows(feat), sigma_params, mode, e_x=to_rows(hn.bound_fwd(mag)))
    ref.feat, ref.mag = feat, mag
    return ref


def evaluate(x, sigma_params, mode="fp32", mutant="none", dt=F64):
    """The same net WITHOUT bounds, in float64 or in plain fp32 with sequential
    sums, optionally with one deliberate mistake -> (h, sigma) as fp32 arrays
    (what a kernel would hand back)."""
    half = mode == "f16"
    p = sn._np(sigma_params, F64)
    x = np.asarray(x, F64).reshape(-1, 32)
    if half:
        p, x = sn.q16(p), sn.q16(x)
    p, x = p.astype(dt), x.astype(dt)
    W1, W2 = p[:2048].reshape(64, 32), p[2048:3072].reshape(16, 64)
    if mutant == "cols_c_major":
        x = np.ascontiguousarray(x.reshape(-1, 16, 2).transpose(0, 2, 1).reshape(-1, 32))
    if mutant == "w2_rows_swapped":
        W2 = W2.copy()
        W2[[0, 1]] = W2[[1, 0]]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a1 = sn._dot(x, W1, dt)
        hid = np.maximum(a1, 0)
        if mutant == "relu_dropped":
            hid[:, 7] = a1[:, 7]
        if half and mutant != "f16_hidden_unrounded":
            hid = sn.q16(hid).astype(dt)
        h = sn._dot(hid, W2, dt)
        if mutant == "tail_block_last_row":
            M = h.shape[0]
            if M % 16:
                h[M // 16 * 16:] = h[M - 1]
        h0 = np.asarray(h[:, 1] if mutant == "sigma_from_h1" else h[:, 0], F64)
        if mutant == "sigma_clamped":
            h0 = np.clip(h0, -15.0, 15.0)
        sigma = np.exp(h0).astype(F32)        # correctly rounded: inside expf's 1 ulp
    return np.asarray(h, F32), sigma


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def compare_density(got_h, got_sigma, ref, what):
    """h through ``shade_numpy.compare`` (|got - ref| <= bound per element, the
    worst ratio recorded in ``WORST``), sigma by membership of its interval.
    A row whose reference is NOT finite (an fp16 feature beyond 65504) has no
    bound: there every element must be of the reference's class -- NaN, +inf or
    -inf, which IEEE sums reach whatever their order -- and sigma NaN, inf or 0
    accordingly.  ``what`` = "<entry point> <family> @ <case>".  -> worst."""
    got_h, got_sigma = sn._np(got_h, F64), sn._np(got_sigma, F64).reshape(-1)
    ref_h = np.asarray(ref.h, F64)
    if got_h.shape != ref_h.shape or got_sigma.shape[0] != ref_h.shape[0]:
        raise sn.Mismatch(f"{what}: shape {got_h.shape} / {got_sigma.shape} != {ref_h.shape}")
    fin = np.isfinite(ref_h).all(1)
    name, _, where = what.partition(" @ ")
    worst = sn.compare(got_h[fin], ref_h[fin], ref.e_h[fin], f"{name} h @ {where}")
    for r in np.nonzero(~fin)[0]:
        g, w = got_h[r], ref_h[r]
        same = (np.isnan(g) == np.isnan(w)) & (np.isposinf(g) == np.isposinf(w)) & \
               (np.isneginf(g) == np.isneginf(w))
        if not same.all():
            raise sn.Mismatch(f"{what}: row {r} overflows in the reference as {w!r}, got {g!r}")
    ok = sn.in_sigma_interval(got_sigma, ref.sigma_lo, ref.sigma_hi)
    if not ok.all():
        i = int(np.argmin(ok))
        raise sn.Mismatch(f"{what}: sigma[{i}] = {got_sigma[i]!r} outside "
                          f"[{ref.sigma_lo[i]!r}, {ref.sigma_hi[i]!r}] ({int((~ok).sum())} rows)")
    return worst


# ---------------------------------------------------------------------------
# cases: net inputs as rows x [M, 32] fp32
# ---------------------------------------------------------------------------
def scaled_weights(seed=5, scale=8.0):
    """one ``mlp_init`` draw of the sigma net x 8: hidden magnitudes differ"""
    import torch
    from oracle import field as ofield
    spec = ofield.MLPSpec(32, 16, 64, 1)
    return (ofield.mlp_init(spec, torch.Generator().manual_seed(seed)).numpy() * scale).astype(F32)


def case_sizes(M, seed=0):
    """x ~ 0.5 N(0, 1); from M = 15 on the middle row is all zero (h = 0 and
    sigma = 1 exactly)."""
    rng = np.random.default_rng(8000 + M + seed)
    x = (0.5 * rng.standard_normal((M, 32))).astype(F32)
    if M >= 15:
        x[M // 2] = 0
    return NS(name=f"sizes[{M}]", M=M, x=x)


MAGNITUDE_EXPONENTS = (-30, -27, -24, -20, -17, -15, -14, -13, -12)


def case_magnitudes(f16=False, seed=0):
    """Three rows N(0, 1) x 2^k for every k of ``MAGNITUDE_EXPONENTS`` (below
    2^-13 an f16x2 operand is no longer relative; below 2^-14 / 2^-25 an fp16
    feature is subnormal / zero), 8 rows U(-1e-4, 1e-4) (the grid's initial
    scale), 8 rows N(0, 1), 4 rows N(0, 1) x 2^10, one all-zero row.  ``f16``:
    besides, two rows whose entries are +-65504 among N(0, 1) ones and one row
    holding 65520, which rounds to inf in fp16 (``overflow_row``)."""
    rng = np.random.default_rng(8100 + seed)
    rows = [rng.standard_normal((3, 32)) * 2.0 ** k for k in MAGNITUDE_EXPONENTS]
    rows.append((rng.random((8, 32)) * 2 - 1) * 1e-4)
    rows.append(rng.standard_normal((8, 32)))
    rows.append(rng.standard_normal((4, 32)) * 1024.0)
    rows.append(np.zeros((1, 32)))
    c = NS(name="magnitudes" + ("_f16" if f16 else ""), overflow_row=None)
    if f16:
        big = rng.standard_normal((3, 32))
        big[0, [3, 17]] = 65504.0, -65504.0
        big[1, [0, 31]] = -65504.0, 65504.0
        big[2, 9] = 65520.0
        rows.append(big)
    c.x = np.concatenate(rows).astype(F32)
    c.M = c.x.shape[0]
    c.zero_row = c.M - 1 - (3 if f16 else 0)
    if f16:
        c.overflow_row = c.M - 1
    return c


def case_exp(sigma_params, seed=0):
    """One row per target of ``EXP_TARGETS``: a random row x with h0(x) of the
    target's sign, rescaled by alpha = target / h0(x) > 0 (the net has no bias:
    h(alpha x) = alpha h(x)); target 0 is the all-zero row.  The reference is
    computed on the fp32 rows as they are, not on the targets."""
    rng = np.random.default_rng(8200 + seed)
    base = 0.5 * rng.standard_normal((256, 32))
    h0 = density_rows(base.astype(F32), sigma_params, "fp32").h[:, 0]
    rows = []
    for t in EXP_TARGETS:
        if t == 0.0:
            rows.append(np.zeros(32))
            continue
        i = int(np.argmax((np.sign(h0) == np.sign(t)) & (np.abs(h0) > 0.3)))
        assert np.sign(h0[i]) == np.sign(t) and abs(h0[i]) > 0.3
        rows.append(base[i].astype(F32).astype(F64) * (t / h0[i]))
        h0[i] = 0.0                                   # every target its own row
    x = np.stack(rows).astype(F32)
    return NS(name="exp", M=x.shape[0], x=x, targets=EXP_TARGETS)


def slots(M, kind, seed=0):
    """int32 [M]: where row m of the feature array lands"""
    if kind == "identity":
        return np.arange(M, dtype=np.int32)
    if kind == "reverse":
        return np.arange(M, dtype=np.int32)[::-1].copy()
    return np.random.default_rng(8300 + M + seed).permutation(M).astype(np.int32)


def case_fused(H, W, T, bound, seed=0):
    """The pixels of an H x W image, row-major: a pinhole camera inside the box;
    every 7th ray starts outside and looks away (it misses the box: all its
    samples clamp onto one face); depths unsorted and ray-dependent, every 11th
    ray's last sample far beyond the exit (clamped onto the far face)."""
    rng = np.random.default_rng(8400 + 1000 * H + 10 * W + T + seed)
    b = float(bound)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xs - W / 2 + 0.5) / max(W, 8), (ys - H / 2 + 0.5) / max(W, 8),
                  np.ones_like(xs, F64)], -1).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([[0.1 * b, -0.2 * b, -0.6 * b]]), (H * W, 1))
    o[::7] = o[::7] + np.array([0.0, 0.0, -1.5 * b])
    d[::7] = d[::7] * np.array([1.0, 1.0, -1.0])
    z = rng.random((H * W, T)) * (1.5 * b) + 0.1 * b
    z[::11, -1] = 3.0 * b
    return NS(name=f"fused[{H}x{W}x{T}]", H=H, W=W, T=T, o=o.astype(F32), d=d.astype(F32),
              z=np.ascontiguousarray(z.astype(F32)))


def tile_walk(H, W, T):
    """A tile order of the N T samples for the CPU side (the kernels' is
    ucsa_tile_depth_order's or ucsa_tile_index_order's; results are ray-major,
    so WHICH order it is cannot matter): 8 x 8 pixel tiles row-major, inside a
    tile (sample, pixel).  -> slot [M] ray-major index, base [M] the tile's
    first position, rank [M] the position inside the tile."""
    slot, base, rank = [], [], []
    n = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            pix = [(y * W + x) for y in range(ty, min(ty + 8, H)) for x in range(tx, min(tx + 8, W))]
            idx = [r * T + s for s in range(T) for r in pix]
            slot += idx
            base += [n] * len(idx)
            rank += list(range(len(idx)))
            n += len(idx)
    return np.asarray(slot, np.int64), np.asarray(base, np.int64), np.asarray(rank, np.int64)


def fused_mutant_rows(ref, levels, bound, table, pts, H, W, T, n_enc, mutant):
    """The net's input rows x [M, 32] (ray-major, float64) as a WRONG fused
    kernel with ``n_enc`` levels encoded inside would assemble them."""
    feat = ref.feat.copy()                               # [16, M, 2]
    if mutant == "fused_level_12_for_8":
        if n_enc <= 8:                                   # levels 8 + g come from feat_ws
            feat[8:12] = ref.feat[12:16]
    elif mutant == "fused_no_tile_base":
        slot, base, rank = tile_walk(H, W, T)
        first = int((base == 0).sum())
        src = slot[np.minimum(rank, first - 1)]          # the same rank of tile 0
        for l in range(n_enc, 16):
            feat[l, slot] = ref.feat[l, src]
    elif mutant == "fused_table_row_late":
        late = [levels[min(l + 1, 15)] if l >= n_enc else levels[l] for l in range(16)]
        feat = hn.encode(late, bound, pts, table)[0]
    else:
        raise KeyError(mutant)
    return to_rows(feat)
