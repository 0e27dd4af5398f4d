"""numpy restatement of hierarchical resampling (include/ucsa_hip.h:
``ucsa_resample``): the float64 yardstick of tests/test_resample_reference_cpu.py
and tests/test_gpu_resample_reference.py (test infrastructure: plain numpy, no
torch op, no GPU, no HIP library).

It is stated from ``oracle/renderer.py`` (``alpha_weights``, ``inverse_cdf``)
and the header comment of ``ucsa_resample``: the uniforms of a ray are sorted
ascending first.  It knows nothing of waves, chunks or sorting networks: one
row per ray, sequential sums.

    delta_i = z_{i+1} - z_i  (the last one 1e10)      x_i = -delta_i scale sigma_i
    alpha_i = 1 - exp(x_i)     fac_i = 1 - alpha_i + 1e-15
    T_i = prod_{j<i} fac_j     w_i = alpha_i T_i
    bins_i = z_i + 0.5 delta_i                          i = 0 .. T-2
    pdf_k = (w_k + 1e-5) / sum_{j=1..T-2} (w_j + 1e-5)  k = 1 .. T-2
    cdf_0 = 0, cdf_k = sum_{j<=k} pdf_j                 T-1 entries
    lo = first index with cdf[lo] > u  (T-1 if none)
    below = max(lo-1, 0), above = min(lo, T-2)
    denom = cdf[above] - cdf[below];  denom < 1e-5 -> 1
    new_z = bins[below] + (u - cdf[below]) / denom (bins[above] - bins[below])

BRANCHES ARE IN THE REFERENCE, NOT IN THE TOLERANCE.  ``lo`` and the ``denom``
guard are discontinuous, and an empty bin's pdf (1e-5 / sum) sits within
round-off of the guard's threshold, so no flat tolerance works.  ``reference``
returns, for every output sample, a SET of allowed intervals (v, e), one per
branch combination that an fp32 evaluation may legitimately take:

* bin index: every ``lo`` with cdf[lo-1] - e_cdf[lo-1] <= u and
  cdf[lo] + e_cdf[lo] > u (a binary search over ANY array, monotone or not,
  ends at an index whose left neighbour it saw <= u and which it saw > u);
* guard: taken where denom - e_denom < 1e-5f, not taken where denom + e_denom
  >= 1e-5f, both where both hold.

The kernel's value must lie in at least one interval; no sample is exempt.

BOUNDS by running error analysis, ``U = 2^-24``, each step from the source
(csrc/sampling.hip, built with -ffp-contract=off: one rounding per operation):

* x: the subtraction and two products: 3 U |x|; exactly 0 where delta or sigma
  is 0 (a product with an exact zero is exact).  ``density_scale`` crosses the
  ABI as a float: the reference uses that fp32 number.
* expf: 1 ulp = 2 U of its value, plus the argument's error pushed through,
  plus one smallest normal number in case a subnormal result is flushed.
* alpha = 1 - expf(x): the exponential's error and one rounding, U alpha: ONE
  ABSOLUTE U near saturation; EXACTLY 0 where x == 0 (expf(0) = 1, 1 - 1 = 0).
* fac: two roundings, 2 U fac, and the constant 1e-15f (U 1e-15 off 1e-15).
* T_i, a product of i factors: the factors' ABSOLUTE errors carried through it,
  prod(fac + e_fac) - prod(fac) (after an opaque sample fac is the bare 1e-15
  while e_fac stays ~U: a relative bound means nothing there, the absolute one
  stays ~U), then i + 2 roundings of the result for i - 1 multiplications in
  ANY association plus the product with alpha's partner and slack: this covers
  the DPP scan's tree and the chunk carry without modelling them.  T_0 = 1
  exactly.
* w = alpha T: both bounds pushed through, one rounding.
* w + 1e-5f: one rounding, and the constant (U 1e-5 off 1e-5).
* the normaliser, a sum of K = T - 2 positive terms in any order: the terms'
  bounds plus (K + 2) U of the sum.
* the quotient: one rounding (fp32 division is correctly rounded), numerator
  and denominator bounds pushed through.
* cdf_k, a sum of k terms in any order: the terms' bounds plus (k + 2) U of the
  sum.  cdf_0 = 0 exactly.
* bins: the subtraction, the exact halving and the addition: U (|delta| + |bins|).
* the interpolation: u - c0 (e_c0 and one rounding) over denom (e_c0 + e_c1 and
  one rounding; >= 1e-5f whenever the guard is not taken, which caps the
  quotient's blow-up) by interval arithmetic -- THE CDF BOUNDS ENTER DIVIDED BY
  denom, the term that matters -- then one rounding each for the quotient, the
  product with bins[above] - bins[below] (two bin bounds and a rounding; exactly
  0 when the clamps make below == above) and the final addition.

``resample(..., dt=F32)`` evaluates the same formulas in fp32 (expf as the
correctly rounded exponential) with its own branches, in three summation /
product orders: ``seq`` sequential, ``scan`` a doubling scan over the whole ray
(every prefix a balanced tree; totals by halving), ``chunk`` doubling scans of
64 chained by a carry.  They serve the test that the bounds are not tighter
than fp32 arithmetic allows.  ``mutant`` names one deliberate mistake for the
sharpness tests (``MUTANTS``).
"""
from types import SimpleNamespace as NS

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24                      # unit round-off of fp32
TINY = 2.0 ** -126                  # smallest normal fp32 number
FLOOR32 = float(F32(1e-5))          # the guard's threshold and the pdf floor as the kernel holds them
LAST_U = float(np.nextafter(F32(1.0), F32(0.0)))
ORDERS = ("seq", "scan", "chunk")
AMBIGUITY_CAP = 0.05

# one deliberate mistake each:
MUTANTS = (
    "carry_lost_64",     # the transmittance carry is dropped at every 64-sample boundary
    "run_lost_64",       # the cdf running sum is dropped at every 64-entry boundary
    "drop_1e5",          # no pdf floor
    "drop_1e15",         # fac = 1 - alpha             (NOT observable in fp32: see EQUIVALENT)
    "wsum_all",          # the normaliser includes the first and the last weight
    "bins_are_z",        # no midpoint
    "last_delta_prev",   # the last interval is as wide as the one before (NOT observable)
    "no_denom_guard",    # denom is used as it is
    "above_unclamped",   # above = lo even past the last entry: cdf[T-1] is the slot the last
                         # WEIGHT was left in, bins[T-1] is never written (indeterminate: NaN)
    "pad_leak",          # a pad value (0) takes part in the sort when t < tpad: the largest
                         # real uniform is lost
    "unsorted",          # output in input order
    "scale_ignored",     # density_scale is treated as 1
)
# Two of them cannot show in this stage's output, whatever the test: 1e-15 only matters where
# 1 - alpha rounds to 0, and everything behind an opaque sample then weighs <= 1e-15 against a
# pdf floor of 1e-5 (1e-10 of ONE rounding of it); the last interval only enters alpha_{T-1},
# and the pdf runs over w_1 .. w_{T-2}.  The tests assert exactly that: inside every interval.
EQUIVALENT = ("drop_1e15", "last_delta_prev")


def _np(a, dtype):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a, dtype))


def _a64(v):
    return np.abs(np.asarray(v, F64))


# ---------------------------------------------------------------------------
# scans and totals in a given order
# ---------------------------------------------------------------------------
def _doubling(x, op):
    """inclusive scan along the last axis, Kogge-Stone: every prefix a balanced tree"""
    d, n = 1, x.shape[-1]
    while d < n:
        y = x.copy()
        y[..., d:] = op(x[..., d:], x[..., :-d])
        x, d = y, 2 * d
    return x


def scan(x, kind, order, lost=False):
    """Inclusive product ("mul") or sum ("add") of x [N, n] along each row in
    x's own dtype.  ``lost``: nothing is carried across a multiple of 64."""
    op, ident = (np.multiply, 1.0) if kind == "mul" else (np.add, 0.0)
    N, n = x.shape
    if n == 0:
        return x.copy()
    if not lost and order == "seq":
        return op.accumulate(x, axis=1, dtype=x.dtype)
    if not lost and order == "scan":
        return _doubling(x, op)
    c = -(-n // 64)
    ch = np.full((N, c * 64), ident, x.dtype)
    ch[:, :n] = x
    ch = ch.reshape(N, c, 64)
    inc = op.accumulate(ch, axis=2, dtype=x.dtype) if order == "seq" else _doubling(ch, op)
    if not lost:
        carry = np.full((N, c), ident, x.dtype)
        for k in range(1, c):
            carry[:, k] = op(carry[:, k - 1], inc[:, k - 1, -1])
        inc = op(carry[:, :, None], inc)
    return inc.reshape(N, c * 64)[:, :n]


def total(x, order):
    """sum of each row: sequentially, or by halving (a butterfly)"""
    N, n = x.shape
    if n == 0:
        return np.zeros(N, x.dtype)
    if order == "seq":
        return np.add.accumulate(x, axis=1, dtype=x.dtype)[:, -1]
    m = 1
    while m < n:
        m *= 2
    p = np.zeros((N, m), x.dtype)
    p[:, :n] = x
    while m > 1:
        m //= 2
        p = p[:, :m] + p[:, m:]
    return p[:, 0]


# ---------------------------------------------------------------------------
# stage 1: weights and bin midpoints
# ---------------------------------------------------------------------------
def ray_weights(z, sigma, density_scale, dt=F64, order="seq", mutant=()):
    """oracle.renderer.alpha_weights and the midpoints, with their bounds (see
    the module docstring).  z, sigma [N, T] -> w [N, T], bins [N, T-1]."""
    z, sg = _np(z, F32).astype(dt), _np(sigma, F32).astype(dt)
    N, T = z.shape
    assert T >= 3
    ds = dt(1.0) if "scale_ignored" in mutant else dt(F32(density_scale))
    with np.errstate(under="ignore", over="ignore"):
        delta = np.empty_like(z)
        delta[:, :-1] = z[:, 1:] - z[:, :-1]
        delta[:, -1] = delta[:, -2] if "last_delta_prev" in mutant else dt(1e10)
        x = -delta * ds * sg
        ex = np.exp(x.astype(F64)).astype(dt)
        alpha = dt(1.0) - ex
        fac = dt(1.0) - alpha
        if "drop_1e15" not in mutant:
            fac = fac + dt(1e-15)
        lost = "carry_lost_64" in mutant
        incl = scan(fac, "mul", order, lost)
        Tr = np.ones_like(z)
        Tr[:, 1:] = incl[:, :-1]
        if lost:
            Tr[:, 64::64] = 1.0
        w = alpha * Tr
        bins = z[:, :-1].copy() if "bins_are_z" in mutant else z[:, :-1] + dt(0.5) * delta[:, :-1]
        # bounds
        x64, ex64, al64, fac64, T64 = (np.asarray(v, F64) for v in (x, ex, alpha, fac, Tr))
        zero = x64 == 0
        e_x = np.where(zero, 0.0, 3.0 * U * np.abs(x64) + TINY)
        e_ex = np.where(zero, 0.0, ex64 * (np.expm1(np.minimum(e_x, 1.0)) + 2.0 * U) + TINY)
        e_alpha = np.where(zero, 0.0, e_ex + U * np.abs(al64))
        e_fac = e_alpha + 2.0 * U * fac64 + U * 1e-15
        e_in = np.zeros((N, T))
        e_in[:, 1:] = (np.multiply.accumulate(fac64 + e_fac, axis=1)
                       - np.multiply.accumulate(fac64, axis=1))[:, :-1]
        i = np.arange(T)
        e_T = e_in + (i + 2) * U * (T64 + e_in) + i * TINY
        e_T[:, 0] = 0.0
        e_w = e_alpha * (T64 + e_T) + np.abs(al64) * e_T + U * _a64(w)
        e_bins = U * (_a64(delta[:, :-1]) + _a64(bins))
    return NS(delta=delta, x=x, ex=ex, alpha=alpha, fac=fac, T=Tr, w=w, bins=bins,
              e_alpha=e_alpha, e_fac=e_fac, e_T=e_T, e_w=e_w, e_bins=e_bins)


# ---------------------------------------------------------------------------
# stage 2: pdf and cdf of the interior weights
# ---------------------------------------------------------------------------
def pdf_cdf(wi, e_wi, dt=F64, order="seq", mutant=(), w_ends=None):
    """wi [N, K] interior weights (w_1 .. w_{T-2}) -> cdf [N, K + 1], e_cdf."""
    wi = np.asarray(wi, dt)
    N, K = wi.shape
    floor = dt(0.0) if "drop_1e5" in mutant else dt(1e-5)
    wp = wi + floor
    src = np.concatenate([wp, np.asarray(w_ends, dt) + floor], 1) if "wsum_all" in mutant else wp
    with np.errstate(divide="ignore", invalid="ignore"):
        wsum = total(src, order)[:, None]
        p = wp / wsum
        p0 = np.concatenate([np.zeros((N, 1), dt), p], 1)
        cdf = scan(p0, "add", order, "run_lost_64" in mutant)
        # bounds
        wp64, p64, cdf64 = (np.asarray(v, F64) for v in (wp, p, cdf))
        e_wp = np.asarray(e_wi, F64) + U * wp64 + U * 1e-5
        S = wp64.sum(1, keepdims=True)
        e_S = e_wp.sum(1, keepdims=True) + (K + 2) * U * S
        S_lo = S - e_S
        e_p = e_wp / S_lo + wp64 * e_S / (S * S_lo) + U * p64
        acc = np.concatenate([np.zeros((N, 1)), np.cumsum(e_p, 1)], 1)
        e_cdf = acc + (np.arange(K + 1) + 2) * U * (cdf64 + acc)
        e_cdf[:, 0] = 0.0
    return NS(p=p, wsum=wsum, cdf=cdf, e_cdf=e_cdf)


# ---------------------------------------------------------------------------
# stage 3: the sorted uniforms and the inversion
# ---------------------------------------------------------------------------
def sorted_uniforms(u, mutant=(), sort=True):
    u = _np(u, F32)
    if not sort or "unsorted" in mutant:
        return u.copy()
    us = np.sort(u, axis=1)
    t = u.shape[1]
    tpad = 2
    while tpad < t:
        tpad *= 2
    if "pad_leak" in mutant and t < tpad:
        us = np.concatenate([np.zeros((u.shape[0], 1), F32), us[:, :-1]], 1)
    return us


def _rows_searchsorted(a, v):
    """first index of row a[r] whose entry is > v[r, q]"""
    return np.stack([np.searchsorted(a[r], v[r], side="right") for r in range(a.shape[0])]) \
        if a.shape[0] else np.zeros(v.shape, np.int64)


def _take(a, idx):
    return np.take_along_axis(a, idx, 1)


def invert(bins, cdf, us, dt=F64, mutant=(), w_last=None):
    """oracle.renderer.inverse_cdf on sorted uniforms, with ITS OWN branches
    (decided in dt).  bins, cdf [N, n], us [N, t] -> new_z [N, t]."""
    bins, cdf, us = np.asarray(bins, dt), np.asarray(cdf, dt), np.asarray(us, dt)
    n = cdf.shape[1]
    lo = _rows_searchsorted(cdf, us)
    below, above = np.maximum(lo - 1, 0), np.minimum(lo, n - 1)
    c0, c1, b0, b1 = _take(cdf, below), _take(cdf, above), _take(bins, below), _take(bins, above)
    if "above_unclamped" in mutant:
        past = lo == n
        c1 = np.where(past, np.asarray(w_last, dt)[:, None], c1)
        b1 = np.where(past, dt(np.nan), b1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        denom = c1 - c0
        if "no_denom_guard" not in mutant:
            denom = np.where(denom < dt(1e-5), dt(1.0), denom)
        return b0 + (us - c0) / denom * (b1 - b0)


def intervals(bins, e_bins, cdf, e_cdf, us):
    """Every (v, e) a legitimate fp32 evaluation may land in: candidates x
    {guard taken, guard not taken}.  -> V, E, OK [C, N, t]."""
    bins, e_bins, cdf, e_cdf, us = (np.asarray(v, F64) for v in (bins, e_bins, cdf, e_cdf, us))
    n = cdf.shape[1]
    # monotone envelopes (cdf +- e_cdf are monotone already unless a bound exceeds a bin)
    hi_env = np.maximum.accumulate(cdf + e_cdf, axis=1)
    lo_env = np.minimum.accumulate((cdf - e_cdf)[:, ::-1], axis=1)[:, ::-1]
    lo_min = _rows_searchsorted(hi_env, us)          # first lo with cdf[lo] + e > u
    lo_max = _rows_searchsorted(lo_env, us)          # last lo with cdf[lo-1] - e <= u
    assert (lo_min <= lo_max).all()
    V, E, OK = [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in range(int((lo_max - lo_min).max()) + 1 if us.size else 0):
            ok = lo_min + c <= lo_max
            lo = np.minimum(lo_min + c, lo_max)
            below, above = np.maximum(lo - 1, 0), np.minimum(lo, n - 1)
            same = below == above
            c0, c1, e0, e1 = _take(cdf, below), _take(cdf, above), _take(e_cdf, below), _take(e_cdf, above)
            b0, b1, eb0, eb1 = _take(bins, below), _take(bins, above), _take(e_bins, below), _take(e_bins, above)
            num = us - c0
            e_num = e0 + U * (np.abs(num) + e0)
            den = c1 - c0
            e_den = np.where(same, 0.0, e0 + e1 + U * (np.abs(den) + e0 + e1))
            db = b1 - b0
            e_db = np.where(same, 0.0, eb0 + eb1 + U * (np.abs(db) + eb0 + eb1))
            n_lo, n_hi = num - e_num, num + e_num
            for taken in (True, False):
                if taken:
                    allowed = ok & (den - e_den < FLOOR32)
                    q_lo, q_hi = n_lo, n_hi                    # denom = 1: the quotient is exact
                    rnd = 0.0
                else:
                    allowed = ok & (den + e_den >= FLOOR32)
                    d_lo = np.maximum(den - e_den, FLOOR32)    # not taken: the kernel's denom >= 1e-5f
                    d_hi = np.maximum(den + e_den, d_lo)
                    q_hi = np.where(n_hi >= 0, n_hi / d_lo, n_hi / d_hi)
                    q_lo = np.where(n_lo >= 0, n_lo / d_hi, n_lo / d_lo)
                    rnd = U
                q = 0.5 * (q_lo + q_hi)
                e_q = 0.5 * (q_hi - q_lo) + rnd * np.maximum(np.abs(q_lo), np.abs(q_hi))
                prod = q * db
                e_prod = (e_q * (np.abs(db) + e_db) + np.abs(q) * e_db
                          + U * (np.abs(q) + e_q) * (np.abs(db) + e_db))
                v = b0 + prod
                e = eb0 + e_prod + U * (np.abs(v) + eb0 + e_prod)
                V.append(np.where(allowed, v, np.nan))
                E.append(np.where(allowed, e, np.nan))
                OK.append(allowed)
    return np.array(V), np.array(E), np.array(OK)


# ---------------------------------------------------------------------------
# the whole stage
# ---------------------------------------------------------------------------
def resample(z, sigma, u, density_scale=1.0, dt=F64, order="seq", mutant=()):
    """new_z [N, t] evaluated in ``dt`` with the evaluation's own branches."""
    rw = ray_weights(z, sigma, density_scale, dt, order, mutant)
    pc = pdf_cdf(rw.w[:, 1:-1], rw.e_w[:, 1:-1], dt, order, mutant, rw.w[:, [0, -1]])
    us = sorted_uniforms(u, mutant)
    return invert(rw.bins, pc.cdf, us, dt, mutant, rw.w[:, -1])


def _finish(bins, e_bins, pc, us):
    V, E, OK = intervals(bins, e_bins, pc.cdf, pc.e_cdf, us)
    n_allowed = OK.sum(0)
    assert (n_allowed >= 1).all()
    return NS(value=invert(bins, pc.cdf, us), V=V, E=E, OK=OK, n_allowed=n_allowed, us=us,
              ambiguous=float((n_allowed > 1).mean()) if n_allowed.size else 0.0,
              bins=bins, cdf=pc.cdf, e_cdf=pc.e_cdf)


def reference(z, sigma, u, density_scale=1.0):
    """The float64 value of every output sample (r, q) of the ascending-sorted
    uniforms and its set of allowed intervals: .value [N, t]; .V, .E, .OK
    [C, N, t]; .n_allowed [N, t]; .ambiguous = the fraction with more than one."""
    rw = ray_weights(z, sigma, density_scale)
    pc = pdf_cdf(rw.w[:, 1:-1], rw.e_w[:, 1:-1])
    ref = _finish(rw.bins, rw.e_bins, pc, sorted_uniforms(u))
    ref.rw = rw
    return ref


def invert_reference(bins, weights, u, sort=False):
    """The inversion stage alone on exact inputs (``inverse_cdf``'s signature:
    bins [N, T-1], interior weights [N, T-2], u [N, t]), in the order of u."""
    bins, w = _np(bins, F32).astype(F64), _np(weights, F32).astype(F64)
    pc = pdf_cdf(w, np.zeros(w.shape))
    return _finish(bins, np.zeros(bins.shape), pc, sorted_uniforms(u, sort=sort))


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


WORST = {}          # case -> worst |got - v| / e seen (the GPU test prints it at the end)


def ratios(got, ref):
    """per sample: the smallest |got - v| / e over its allowed intervals
    (0 / 0 = 0, x / 0 = inf, non-finite = inf)"""
    got = _np(got, F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got[None] - ref.V)
        r = np.where(err == 0.0, 0.0, err / ref.E)
    r = np.where(ref.OK & ~np.isnan(r), r, np.inf)
    return r.min(0)


def check(got, ref, what):
    """Every sample of ``got`` inside one of its allowed intervals; prints the
    worst ratio, raises above 1.  -> worst."""
    got = _np(got, F64)
    if got.shape != ref.value.shape:
        raise Mismatch(f"{what}: shape {got.shape} != {ref.value.shape}")
    r = ratios(got, ref)
    worst = float(r.max()) if r.size else 0.0
    print(f"{what}: worst |got - v| / e {worst:.3f}, {ref.ambiguous:.2%} of the samples with more than one interval")
    WORST[what] = max(WORST.get(what, 0.0), worst)
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(r)), r.shape)
        raise Mismatch(f"{what}: sample {i} = {got[i]!r} outside its {int(ref.n_allowed[i])} interval(s), "
                       f"float64 value {ref.value[i]!r}, nearest at {worst:.3g} of its bound")
    return worst


def caught(got, ref):
    """would the GPU test reject ``got``: a sample outside every interval (a
    non-finite one included) or a ray that does not ascend"""
    got = _np(got, F64)
    return bool((ratios(got, ref) > 1.0).any() or (np.diff(got, axis=1) < 0).any())


# ---------------------------------------------------------------------------
# cases: (T, t) for every chunk situation and sort path, fields and uniforms
# crossed sparingly.  N in {1, 3, 5, 9}: the 4-wave workgroup partial, whole,
# whole plus one; 64 rays where a field needs variety.
# ---------------------------------------------------------------------------
SHARP = ("random", "sparse90", "x50", "spike")
#        name              T     t     N   field        uniforms  density_scale
CASES = (
    ("T3_t1",              3,    1,    9, "random",    "random",  1.0),
    ("T3_t5",              3,    5,    9, "random",    "random",  0.7),
    ("T3_t5_spike",        3,    5,    5, "spike",     "dup",     1.0),
    ("T4_t2_flat",         4,    2,    1, "zero",      "cdfhit",  1.0),
    ("T4_t2",              4,    2,    5, "random",    "random",  3.0),
    ("T16_t3",             16,   3,    9, "sparse90",  "random",  3.0),
    ("T16_t3_x50",         16,   3,    3, "x50",       "desc",    1.0),
    ("T63_t63",            63,   63,   5, "random",    "dup",     1.0),
    ("T64_t64",            64,   64,   9, "x50",       "random",  1.0),
    ("T64_t64_zero",       64,   64,   3, "zero",      "planted", 1.0),
    ("T65_t40",            65,   40,   3, "random",    "asc",     0.7),
    ("T65_t40_spike",      65,   40,   5, "spike",     "desc",    1.0),
    ("T65_t40_tight",      65,   40,   1, "tightz",    "random",  1.0),
    ("T66_t65",            66,   65,   9, "sparse90",  "planted", 0.7),
    ("T128_t100",          128,  100,  5, "random",    "random",  1.0),
    ("T129_t128",          129,  128,  9, "spike",     "random",  3.0),
    ("T129_t128_zmax",     129,  128,  3, "zmax",      "random",  1.0),
    ("T130_t129",          130,  129,  5, "random",    "planted", 1.0),
    ("T96_t200",           96,   200,  9, "x50",       "dup",     0.7),
    ("T96_t200_thr",       96,   200,  3, "threshold", "equal",   1.0),
    ("T256_t256",          256,  256,  64, "sparse90", "random",  1.0),
    ("T256_t256_random",   256,  256,  9, "random",    "planted", 1.0),
    ("T16_t257",           16,   257,  5, "random",    "random",  1.0),
    ("T16_t257_zequal",    16,   257,  1, "zequal",    "desc",    1.0),
    ("T65_t300",           65,   300,  9, "sparse90",  "planted", 3.0),
    ("T300_t512",          300,  512,  3, "random",    "random",  0.7),
    ("T300_t512_zero",     300,  512,  5, "zero",      "dup",     1.0),
    ("T700_t1000",         700,  1000, 5, "spike",     "random",  1.0),
    ("T700_t1000_thr",     700,  1000, 3, "threshold", "low",     1.0),
    ("T1024_t1024",        1024, 1024, 9, "spike",     "planted", 0.7),
    ("T1024_t1024_zmax",   1024, 1024, 3, "zmax",      "asc",     1.0),
    # more than 64 KiB of LDS
    ("T1024_t1025",        1024, 1025, 5, "spike",     "random",  1.0),
    ("T1024_t1025_sparse", 1024, 1025, 3, "sparse90",  "planted", 3.0),
    ("T2048_t1024",        2048, 1024, 3, "spike",     "dup",     1.0),
    ("T2048_t1024_tight",  2048, 1024, 1, "tightz",    "random",  1.0),
)
CASE_NAMES = tuple(c[0] for c in CASES)


def _field(kind, rng, N, T, ds):
    """-> z, sigma [N, T] fp32"""
    z = np.sort(0.2 + 7.0 * rng.random((N, T)), 1).astype(F32)
    dens = (3.0 * rng.random((N, T))) ** 3
    delta = np.diff(z.astype(F64), axis=1)
    rows = np.arange(N)
    if kind == "random":
        sigma = dens
    elif kind == "sparse90":
        sigma = np.where(rng.random((N, T)) < 0.9, 0.0, dens)
    elif kind == "x50":
        # alpha saturates: 1 - alpha + 1e-15 is the bare floor and the product underflows.
        # Every other ray starts transparent, so that the saturation happens among the
        # interior weights and not before them
        sigma = 50.0 * dens
        sigma[::2, 0] = 0.0
    elif kind in ("spike", "threshold"):
        # one interior sample: half opaque (the pdf's empty bins are clearly above the
        # guard's threshold), or opaque late in the ray (the interior weights sum to 1:
        # every empty bin sits just below it)
        j = rng.integers(1, T - 1, N) if kind == "spike" else rng.integers(max(1, (T - 1) // 2), T - 1, N)
        sigma = np.zeros((N, T))
        sigma[rows, j] = (np.log(2.0) if kind == "spike" else 200.0) / (delta[rows, j] * ds)
    elif kind == "zero":
        sigma = np.zeros((N, T))
    elif kind == "tightz":
        # spacing ~1e-6 of the depth: a dozen ulps
        z = (3.0 + np.cumsum(3e-6 * (0.7 + 0.6 * rng.random((N, T))), 1)).astype(F32)
        sigma = dens * 1e5
    elif kind == "zequal":
        z = np.full((N, T), 2.5, F32)
        sigma = dens
    elif kind == "zmax":
        # what a ray that misses the box gets
        z = np.full((N, T), 3.4028235e38, F32)
        sigma = dens
    else:
        raise KeyError(kind)
    return z, sigma.astype(F32)


def _uniforms(kind, rng, N, T, t):
    u = rng.random((N, t)).astype(F32)
    u = np.minimum(u, F32(LAST_U))
    if kind == "random":
        pass
    elif kind == "planted":
        # 0 and the largest fp32 number below 1 (it can exceed an fp32 cdf that ends below 1)
        if t >= 2:
            u[:, 0], u[:, -1] = 0.0, LAST_U
        else:
            u[::2, 0], u[1::2, 0] = 0.0, LAST_U
    elif kind == "dup":
        u[:, 1::2] = u[:, 0:2 * (t // 2):2]
    elif kind == "equal":
        u[:] = u[:, :1]
        u[0] = 0.5
    elif kind == "asc":
        u = np.sort(u, 1)
    elif kind == "desc":
        u = np.sort(u, 1)[:, ::-1].copy()
    elif kind == "cdfhit":
        # values equal to an entry of a flat pdf's cdf: k / (T - 2)
        u = np.broadcast_to(((np.arange(t) + 1) % (T - 2) / (T - 2)).astype(F32), (N, t)).copy()
    elif kind == "low":
        # a quarter of them in the first thousandth of the cdf
        u[:, ::4] *= F32(1e-3)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(u, F32)


def build_case(name):
    """-> NS(name, T, t, N, z, sigma, u, density_scale, sharp)"""
    k = CASE_NAMES.index(name)
    _, T, t, N, field, unif, ds = CASES[k]
    rng = np.random.default_rng(9000 + k)
    z, sigma = _field(field, rng, N, T, ds)
    return NS(name=name, T=T, t=t, N=N, field=field, uniforms=unif, density_scale=ds,
              z=z, sigma=sigma, u=_uniforms(unif, rng, N, T, t), sharp=field in SHARP)
