"""numpy restatement of the multiresolution hash-grid encode and of its table
gradient (include/ucsa_hip.h: ``ucsa_hashgrid_encode_*``, ``ucsa_hashgrid_bwd_*``),
the float64 yardstick of tests/test_hashgrid_reference_cpu.py and
tests/test_gpu_hashgrid_reference.py (test infrastructure: plain numpy, no
torch op, no GPU, no HIP library).  It knows nothing of waves, runs, bins or
records: one contribution per (sample, corner), summed.

Two precisions on purpose:

* the POSITION, the cell and the fractional part are fp32, one operation per
  line in the kernels' order (the library is built with -ffp-contract=off and
  these stages are elementwise), so the reference lands in the kernel's cell and
  sees the kernel's ``frac`` bit for bit.  A float64 position would flip cells
  at boundaries, and no tolerance would mean anything;
* from ``frac`` on everything is float64: weights, products, sums.

The level table comes from the caller as ``(scale, res, entries, offset,
hashed)`` rows (``levels_of``): nothing about a particular grid is written down
here.

The last part builds the inputs both test files share (numpy generators, fp32
arrays): the smallest shapes at which the kernels can still go wrong.

The ``bound_*`` functions are the per-element error budgets of the fp32 kernels
against these float64 values, from counting rounding steps; ``u = 2^-24``.
"""
import math

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24                    # unit round-off of fp32
PRIME_Y = 2654435761
PRIME_Z = 805459861
M32 = 0xFFFFFFFF
BIN_COUNT = 256                   # bins per level of the two-pass backward
BIN_SCALE = 100.0                 # default of UCSA_BWD_BIN_SCALE


def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype))


# ---------------------------------------------------------------------------
# level table
# ---------------------------------------------------------------------------
def levels_of(src):
    """-> [(scale, res, entries, offset, hashed)] from the ``Grid`` struct, from
    ``encoder.level_table()`` (dicts) or from the oracle's ``GridSpec``."""
    if hasattr(src, "n_levels") and hasattr(src, "level"):          # ctypes Grid
        rows = [src.level[l] for l in range(int(src.n_levels))]
    elif hasattr(src, "levels"):                                    # GridSpec
        rows = list(src.levels)
    else:
        rows = list(src)
    out = []
    for r in rows:
        get = (lambda k, r=r: r[k]) if isinstance(r, dict) else (lambda k, r=r: getattr(r, k))
        out.append((float(get("scale")), int(get("res")), int(get("entries")),
                    int(get("offset")), bool(get("hashed"))))
    return out


def total_entries(levels):
    return levels[-1][3] + levels[-1][2]


def binned_levels(levels, with_workspace=True, bin_scale=BIN_SCALE):
    """bool per level: goes through the LDS bins (host code of the backward: the
    first hashed level with scale >= bin_scale and every level after it)."""
    n_lo = len(levels)
    if with_workspace:
        n_lo = 0
        while n_lo < len(levels) and (not levels[n_lo][4] or levels[n_lo][0] < bin_scale):
            n_lo += 1
    return np.arange(len(levels)) >= n_lo


# ---------------------------------------------------------------------------
# positions: fp32, the kernels' order of operations
# ---------------------------------------------------------------------------
def ray_points(rays_o, rays_d, z, aabb):
    """p = clamp(o + d * z, lo, hi) -> [N*T, 3] fp32 (ray-major)."""
    o = _np(rays_o, F32).reshape(-1, 3)
    d = _np(rays_d, F32).reshape(-1, 3)
    z = _np(z, F32)
    assert z.ndim == 2 and z.shape[0] == o.shape[0] == d.shape[0]
    aabb = np.asarray(aabb, F32)
    prod = d[:, None, :] * z[:, :, None]
    p = o[:, None, :] + prod
    p = np.maximum(p, aabb[:3])
    p = np.minimum(p, aabb[3:])
    assert p.dtype == F32
    return np.ascontiguousarray(p.reshape(-1, 3))


def unit_coords(points, bound):
    """x01 = (p + bound) * (1 / (2 bound)) when 2 bound is a power of two, else
    (p + bound) / (2 bound); fp32."""
    p = _np(points, F32).reshape(-1, 3)
    b = F32(bound)
    two_b = F32(2.0) * b
    s = p + b
    mant, _ = math.frexp(float(two_b))
    if mant == 0.5:
        x01 = s * (F32(1.0) / two_b)
    else:
        x01 = s / two_b
    assert x01.dtype == F32
    return x01


def cell_frac(x01, scale):
    """pos = x01 * scale + 0.5f; -> (cell int64 [M,3], frac fp32 [M,3])."""
    pos = x01 * F32(scale)
    pos = pos + F32(0.5)
    cell = np.floor(pos)
    frac = pos - cell
    assert frac.dtype == F32
    return cell.astype(np.int64), frac


# ---------------------------------------------------------------------------
# corners: float64 weights, uint32 index arithmetic
# ---------------------------------------------------------------------------
def corner_index(level, gx, gy, gz):
    """Global table entry of corner (gx, gy, gz) on ``level``: uint32 arithmetic
    carried in uint64, then ``% entries``, then ``+ offset``."""
    _, res, entries, offset, hashed = level
    gx = np.asarray(gx, np.uint64) & np.uint64(M32)
    gy = np.asarray(gy, np.uint64) & np.uint64(M32)
    gz = np.asarray(gz, np.uint64) & np.uint64(M32)
    if hashed:
        idx = gx ^ ((gy * np.uint64(PRIME_Y)) & np.uint64(M32)) ^ \
            ((gz * np.uint64(PRIME_Z)) & np.uint64(M32))
    else:
        idx = (gx + gy * np.uint64(res) + gz * np.uint64(res * res)) & np.uint64(M32)
    return (idx % np.uint64(entries)).astype(np.int64) + offset


def corner_weights(frac):
    """w [M, 8] float64: corner c takes frac in dimension d where bit d of c is
    set, 1 - frac otherwise (bit 0 = x)."""
    f = np.asarray(frac, F64)
    one_minus = 1.0 - f
    w = np.empty((f.shape[0], 8), F64)
    for c in range(8):
        w[:, c] = ((f[:, 0] if c & 1 else one_minus[:, 0]) *
                   (f[:, 1] if c & 2 else one_minus[:, 1]) *
                   (f[:, 2] if c & 4 else one_minus[:, 2]))
    return w


def level_corners(levels, bound, points):
    """Per level (idx [M, 8] int64 global entries, w [M, 8] float64, frac [M, 3]
    fp32)."""
    x01 = unit_coords(points, bound)
    out = []
    for level in levels:
        cell, frac = cell_frac(x01, level[0])
        idx = np.empty((cell.shape[0], 8), np.int64)
        for c in range(8):
            idx[:, c] = corner_index(level, cell[:, 0] + (c & 1), cell[:, 1] + ((c >> 1) & 1),
                                     cell[:, 2] + ((c >> 2) & 1))
        out.append((idx, corner_weights(frac), frac))
    return out


# ---------------------------------------------------------------------------
# encode
# ---------------------------------------------------------------------------
def encode_from(corners, table):
    """-> feat [L, M, 2], mag [L, M, 2] = sum_c w_c |v_c| (float64)."""
    if hasattr(table, "detach"):
        table = table.detach().cpu().numpy()
    tab = np.asarray(table).reshape(-1, 2)               # widened after the gather
    feat, mag = [], []
    for idx, w, _ in corners:
        v = tab[idx].astype(F64)                         # [M, 8, 2]
        feat.append((w[:, :, None] * v).sum(1))
        mag.append((w[:, :, None] * np.abs(v)).sum(1))
    return np.stack(feat), np.stack(mag)


def encode(levels, bound, points, table):
    return encode_from(level_corners(levels, bound, points), table)


# ---------------------------------------------------------------------------
# table gradient
# ---------------------------------------------------------------------------
class TableGrad:
    """Sparse table gradient: ``idx`` [K] ascending global entries, ``g`` [K, 2]
    = sum w d_feat, ``A`` [K, 2] = sum w |d_feat|, ``n`` [K] contributions from
    samples whose d_feat pair is not (0, 0), ``level`` [K]."""

    def __init__(self, idx, g, A, n, level):
        self.idx, self.g, self.A, self.n, self.level = idx, g, A, n, level

    def dense(self, total, dtype=F64):
        t = np.zeros((total, 2), dtype)
        t[self.idx] = self.g
        return t


def grad_from(corners, d_feat):
    """Sparse accumulation: ``np.unique`` on the touched entries, ``np.bincount``
    on the compacted ones -- the cost follows the samples, not the table."""
    d_feat = _np(d_feat, F64)
    assert d_feat.ndim == 3 and d_feat.shape[0] == len(corners) and d_feat.shape[2] == 2
    I, G, A, N, L = [], [], [], [], []
    for l, (idx, w, _) in enumerate(corners):
        assert d_feat.shape[1] == idx.shape[0], "d_feat must be [L, M, 2]"
        df = d_feat[l]
        act = ~((df[:, 0] == 0.0) & (df[:, 1] == 0.0))
        ia, wa, da = idx[act].reshape(-1), w[act].reshape(-1), np.repeat(df[act], 8, axis=0)
        uniq, inv = np.unique(ia, return_inverse=True)
        k = uniq.shape[0]
        g = np.stack([np.bincount(inv, wa * da[:, f], k) for f in (0, 1)], 1)
        a = np.stack([np.bincount(inv, wa * np.abs(da[:, f]), k) for f in (0, 1)], 1)
        I.append(uniq)
        G.append(g.reshape(k, 2))
        A.append(a.reshape(k, 2))
        N.append(np.bincount(inv, minlength=k).astype(np.int64))
        L.append(np.full(k, l, np.int64))
    return TableGrad(np.concatenate(I), np.concatenate(G), np.concatenate(A),
                     np.concatenate(N), np.concatenate(L))


def grad(levels, bound, points, d_feat):
    return grad_from(level_corners(levels, bound, points), d_feat)


def grad_rays(levels, bound, rays_o, rays_d, z, aabb, d_feat):
    return grad(levels, bound, ray_points(rays_o, rays_d, z, aabb), d_feat)


def grad_merged(levels, bound, rays_o, rays_d, z_c, z_f, aabb, d_feat_c, d_feat_f):
    """Both density passes: the sum of the two single-pass gradients (the merged
    walk's ``src`` order does not enter)."""
    pts = np.concatenate([ray_points(rays_o, rays_d, z_c, aabb),
                          ray_points(rays_o, rays_d, z_f, aabb)])
    d = np.concatenate([_np(d_feat_c, F64), _np(d_feat_f, F64)], axis=1)
    return grad(levels, bound, pts, d)


def grad_fp32_sequential(corners, d_feat, total):
    """The same formula in plain fp32, accumulated one contribution at a time in
    sample order (``np.add.at`` on a float32 table): what an unoptimised fp32
    implementation gives, the sanity check of the bounds."""
    d_feat = _np(d_feat, F32)
    table = np.zeros((total, 2), F32)
    for l, (idx, _, frac) in enumerate(corners):
        df = d_feat[l]
        act = ~((df[:, 0] == 0.0) & (df[:, 1] == 0.0))
        w = corner_weights_f32(frac)[act]
        for f in (0, 1):
            np.add.at(table[:, f], idx[act].reshape(-1), (w * df[act][:, f:f + 1]).reshape(-1))
    return table


def corner_weights_f32(frac):
    """The kernels' fp32 weights: ((1 * wx') * wy') * wz' in dimension order."""
    f = np.asarray(frac, F32)
    om = F32(1.0) - f
    w = np.empty((f.shape[0], 8), F32)
    for c in range(8):
        t = f[:, 0] if c & 1 else om[:, 0]
        t = t * (f[:, 1] if c & 2 else om[:, 1])
        t = t * (f[:, 2] if c & 4 else om[:, 2])
        w[:, c] = t
    return w


# ---------------------------------------------------------------------------
# error budgets
# ---------------------------------------------------------------------------
def bound_fwd(mag, feat=None, half_features=False):
    """fp32 gather: a weight carries <= 5 roundings (three 1 - f, two products),
    w * v one, the sequential 8-term sum <= 8: |got - feat64| <= 16 u mag.
    fp16 features add the final rounding to half: 2^-11 |feat64| + 2^-25."""
    b = 16.0 * U * np.asarray(mag, F64)
    if half_features:
        b = b + 2.0 ** -11 * np.abs(np.asarray(feat, F64)) + 2.0 ** -25
    return b


def bound_bwd(ref):
    """fp32 paths: 6 roundings per contribution (three 1 - f, two products,
    w * d_feat) and a sum of n terms in ANY order: gamma_k A, k = n + 6."""
    k = (ref.n + 6).astype(F64)[:, None] * U
    return k / (1.0 - k) * ref.A


def bound_bwd_h16(ref, levels, rec_scale):
    """half2 x rec_scale records on the binned levels: + 2^-11 A (rounding to
    half) + n 2^-25 / rec_scale (contributions in the half subnormals)."""
    binned = binned_levels(levels)[ref.level][:, None]
    extra = 2.0 ** -11 * ref.A + ref.n[:, None] * (2.0 ** -25 / rec_scale)
    return bound_bwd(ref) + np.where(binned, extra, 0.0)


def p64_value_bits(entries):
    L = 0
    while (1 << L) < -(-entries // BIN_COUNT):
        L += 1
    return min(32, (64 - L) // 2)


def bound_bwd_p64(ref, levels):
    """Packed records on the binned levels: values rounded to their top V bits
    (sign, 8 exponent bits, V - 9 of the mantissa): + 2^-(V-8) A."""
    binned = binned_levels(levels)
    rel = np.array([2.0 ** -(p64_value_bits(lv[2]) - 8) if b else 0.0
                    for lv, b in zip(levels, binned)])
    return bound_bwd(ref) + rel[ref.level][:, None] * ref.A


def bound_bwd_det(ref):
    """Fixed-point path: the fp32 product w * d_feat (6 roundings), its rounding
    to a multiple of 2^-44 (half a unit each), exact integer sums, one rounding
    of the total to fp32."""
    return 6.0 * U * ref.A + ref.n[:, None] * 2.0 ** -45 + U * np.abs(ref.g)


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def worst_ratio(err, bound):
    """max err / bound with 0 / 0 = 0 and x / 0 = inf."""
    err, bound = np.asarray(err, F64), np.asarray(bound, F64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())


def compare_features(got, feat, bound, what=""):
    """Shapes must match; every element within its bound.  -> worst err / bound."""
    got = _np(got, F64)
    assert got.shape == feat.shape, f"{what}: shape {got.shape} != {feat.shape}"
    assert np.isfinite(got).all(), f"{what}: non-finite features"
    worst = worst_ratio(np.abs(got - feat), bound)
    print(f"{what}: worst err/bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: err/bound {worst:.3g}"
    return worst


def compare_table(got, ref, bound, prior=0.0, what="", one_add=True):
    """The WHOLE table ``got`` [total, 2] against the sparse reference: an entry
    nobody touched keeps exactly ``prior``; a touched one is within ``bound`` of
    prior + g.  A non-zero prior adds the rounding of the addition to it:
    u (|prior| + |g|) when the gradient reaches the entry in ONE addition
    (``one_add``: an entry with a single contribution, or a path whose sums are
    complete before they meet the table); otherwise an entry may be added to
    once per contribution (float atomics from several workgroups), each rounding
    a value of at most |prior| + A: n u (|prior| + A), the same at n = 1.
    -> worst err / bound."""
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    got = np.asarray(got).reshape(-1, 2)
    assert np.isfinite(got).all(), f"{what}: non-finite table gradient"
    changed = (got != got.dtype.type(prior)).any(1)
    changed[ref.idx] = False
    stray = int(np.count_nonzero(changed))
    assert stray == 0, f"{what}: {stray} untouched entries changed"
    b = np.asarray(bound, F64)
    if prior != 0.0 and one_add:
        b = b + U * (abs(prior) + np.abs(ref.g))
    elif prior != 0.0:
        b = b + ref.n[:, None] * U * (abs(prior) + ref.A)
    worst = worst_ratio(np.abs(got[ref.idx].astype(F64) - (prior + ref.g)), b)
    print(f"{what}: worst err/bound {worst:.3f} (max n {int(ref.n.max()) if ref.n.size else 0})")
    assert worst <= 1.0, f"{what}: err/bound {worst:.3g}"
    return worst


# ---------------------------------------------------------------------------
# shared inputs
# ---------------------------------------------------------------------------
def aabb_of(bound):
    return [-float(bound)] * 3 + [float(bound)] * 3


def points_box(M, bound, seed):
    """M random points of the box."""
    rng = np.random.default_rng(seed)
    return ((rng.random((M, 3)) * 2.0 - 1.0) * bound).astype(F32)


def points_faces(bound, seed=1):
    """~600 points: the 8 box corners; one, two and three coordinates at exactly
    +-bound; the origin and points with single zero coordinates (frac = 0 exactly
    on the odd-integer-scale levels: zero weights); random interior points."""
    rng = np.random.default_rng(seed)
    b = float(bound)
    inner = lambda n: (rng.random((n, 3)) * 2.0 - 1.0) * (0.98 * b)   # noqa: E731
    pts = [np.array([[sx * b, sy * b, sz * b] for sx in (-1, 1) for sy in (-1, 1)
                     for sz in (-1, 1)])]
    for axis in range(3):                       # one coordinate on a face
        for sign in (-1.0, 1.0):
            p = inner(20)
            p[:, axis] = sign * b
            pts.append(p)
    for a0, a1 in ((0, 1), (0, 2), (1, 2)):     # two: the 12 edges
        for s0 in (-1.0, 1.0):
            for s1 in (-1.0, 1.0):
                p = inner(10)
                p[:, a0], p[:, a1] = s0 * b, s1 * b
                pts.append(p)
    pts.append(np.zeros((1, 3)))
    for axis in range(3):                       # single zero coordinates
        p = inner(10)
        p[:, axis] = 0.0
        pts.append(p)
    p = inner(6)
    p[:3, :2] = 0.0                             # two zero coordinates
    p[3:, 0], p[3:, 1] = 0.0, b                 # a zero and a face
    pts.append(p)
    n = sum(x.shape[0] for x in pts)
    pts.append(inner(609 - n))
    return np.concatenate(pts).astype(F32)


def points_one_cell(levels, bound, M=4099, seed=2, anchor=(0.3, -1.2, 2.0)):
    """M points inside ONE cell of the finest level (the one holding ``anchor``
    scaled to the box)."""
    rng = np.random.default_rng(seed)
    scale = max(lv[0] for lv in levels)
    a = np.asarray(anchor, F64) * (bound / 4.0)
    k = np.floor((a + bound) / (2.0 * bound) * scale + 0.5)
    centre = k / scale * (2.0 * bound) - bound        # pos = k + 0.5
    width = 2.0 * bound / scale
    return (centre + (rng.random((M, 3)) - 0.5) * (0.8 * width)).astype(F32)


def unit_dirs(rng, n):
    d = rng.standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def d_feat_for(L, M, seed, magnitude=1.0, zeros=True):
    """[L, M, 2] N(0, 1) x magnitude; every 9th sample from the 6th is (0, 0)
    (zero gradients inside runs), and one stretch of 64 consecutive samples."""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((L, M, 2)) * magnitude).astype(F32)
    if zeros and M > 9:
        d[:, 5::9] = 0.0
        if M >= 1200:
            d[:, 1000:1064] = 0.0
    return d


def rays_case(bound, N=37, T=70, seed=3):
    """N rays x T ascending depths (wave boundaries fall mid-ray): rays 0-4
    identical with all z equal (one run of 5 T samples across ray and wave
    boundaries); rays that start outside the box and depths beyond the exit
    (samples clamp onto near and far faces); duplicated depths."""
    rng = np.random.default_rng(seed)
    b = float(bound)
    o = (rng.random((N, 3)) * 2.0 - 1.0) * (0.5 * b)
    d = unit_dirs(rng, N)
    z = np.sort(rng.random((N, T)) * (1.4 * b) + 0.05 * b, axis=1)
    out = slice(5, 12)                              # start outside, look inwards
    o[out] = -d[out] * (1.9 * b)
    z[out] = np.sort(rng.random((7, T)) * (3.5 * b) + 0.2 * b, axis=1)
    z[12:16, T // 2:] += 2.0 * b                    # far beyond the exit
    z[:, 1::16] = z[:, 0::16][:, :z[:, 1::16].shape[1]]     # duplicates
    o[:5], d[:5] = o[0], d[0]
    z[:5] = 0.37 * b
    return o.astype(F32), d.astype(F32), np.ascontiguousarray(z.astype(F32))


def merged_case(bound, N=33, Tc=24, Tf=40, seed=4):
    """Coarse depths spread along the ray, fine ones piled on a "surface";
    duplicates; identical rays; ``src`` = stable sort of the concatenated depths."""
    rng = np.random.default_rng(seed)
    b = float(bound)
    o = (rng.random((N, 3)) * 2.0 - 1.0) * (0.5 * b)
    d = unit_dirs(rng, N)
    z_c = np.sort(0.075 * b + 1.25 * b * np.linspace(0, 1, Tc)[None] +
                  0.0025 * b * rng.random((N, Tc)), axis=1)
    centre = rng.random((N, 1)) * (0.75 * b) + 0.125 * b
    spread = 10.0 ** (-(rng.random((N, 1)) * 2 + 1)) * (b / 4.0)
    z_f = np.maximum(centre + spread * rng.standard_normal((N, Tf)), 0.06 * b)
    z_f[:, 1::8] = z_f[:, 0::8][:, :z_f[:, 1::8].shape[1]]
    z_f = np.sort(z_f, axis=1)
    z_f[3] = z_f[3, 0]                               # one ray: all fine samples equal
    o[::5], d[::5] = o[0], d[0]
    z_c, z_f = z_c.astype(F32), z_f.astype(F32)
    src = np.argsort(np.concatenate([z_c, z_f], 1), axis=1, kind="stable").astype(np.int32)
    return (o.astype(F32), d.astype(F32), np.ascontiguousarray(z_c),
            np.ascontiguousarray(z_f), np.ascontiguousarray(src))


def image_case(bound, H=16, W=24, T=9, seed=5):
    """The pixels of an H x W image (row-major rays) with unsorted, ray-dependent
    depths, some beyond the box."""
    rng = np.random.default_rng(seed)
    b = float(bound)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xs - W / 2 + 0.5) / W, (ys - H / 2 + 0.5) / W, np.ones_like(xs, F64)], -1)
    d = d.reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.tile(np.array([[0.1 * b, -0.2 * b, -0.6 * b]]), (H * W, 1))
    z = rng.random((H * W, T)) * (1.5 * b) + 0.1 * b
    z[::11, -1] = 3.0 * b                            # clamped onto the far face
    return o.astype(F32), d.astype(F32), np.ascontiguousarray(z.astype(F32))


def sparse_rays_case(bound, seed=6):
    """5 rays x 4 samples on a lattice 1.4 / 8 of the box apart: no two samples
    share a corner on any dense level, so every touched entry receives exactly
    one contribution (the callers assert n = 1).  -> (o, d, z)."""
    b = float(bound)
    o = np.array([[-0.875 * b, (-0.75 + 0.375 * i) * b, (0.05 + 0.0025 * i) * b] for i in range(5)])
    d = np.tile(np.array([[1.0, 0.0, 0.0]]), (5, 1))
    z = np.tile((0.125 + 0.35 * np.arange(4))[None] * b, (5, 1))
    return o.astype(F32), d.astype(F32), np.ascontiguousarray(z.astype(F32))
