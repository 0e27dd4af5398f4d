"""Float64 restatement of ``ucsa_augment`` (csrc/augment.hip: ``k_aug_grey_sum``
and ``k_aug_apply``) in NumPy, with a bound per output value that is derived by
counting rounding steps and not fitted to anything.  No torch here, so this
file cannot share a mistake with oracle/augment.py.

Contract restated: ColorJitter's four ops in the drawn ``order`` (0 brightness,
1 contrast, 2 saturation, 3 hue; torchvision 0.12 tensor arithmetic), the mean
grey level taken of the image AS IT ENTERS the contrast op, rotation by the
inverse matrix whose cos / sin are computed in double and rounded to float32,
bilinear sampling with zero padding times the sampled ones-mask, nearest label
with fill -1, crop, horizontal flip.  Inputs are float32; factors and the angle
are float32 values (they cross the C boundary as ``float``); everything after
that is float64.  Non-finite values propagate as in torch: a NaN is not clamped
away, ``max`` / ``min`` hand it on, ``0 * NaN`` is NaN at an in-frame corner.

Rounding count (u = 2^-24, one unit per float32 operation, each in units of the
magnitude of its result; docs/DESIGN_NOTEBOOK.md, section AR, has the same):

* blend(a, b, f) = clamp(f a + (1 - f) b): product, ``1 - f``, product, sum:
  ``u (2 |f a| + 3 |(1 - f) b|)`` on top of ``|f| e_a + |1 - f| e_b``; the
  clamp is 1-Lipschitz and adds nothing.
* grey = 0.2989 r + 0.587 g + 0.114 b: coefficient to float32, product, two
  sums: ``4 u sum |terms|`` on top of the coefficients times the errors.
* mean: the grey errors averaged, plus ``(2 + ceil(log2 P)) u mean|grey|`` for
  a pairwise float32 sum, its division and its rounding (a double sum rounded
  once, as the kernel's, needs 1 of them).
* hue: with e* the largest incoming channel error, v = maxc, cr = maxc - minc,
  the outputs are v, p = v (1 - s), q = v (1 - s f), t = v (1 - s (1 - f)).
  ``v e_s = e_cr + s e_v + u s v <= 3 e* + 2 u v`` (subtraction, division by
  maxc).  ``cr e_(6h) <= 8 e* + 16 u cr`` (two quotients by cr, each
  ``(2 e* + u cr + e_cr) + u cr``, their difference, the offsets 2 or 4) and
  the chain /6, +1, +hue, -floor, *6 adds ``39 u`` to 6h: ``cr e_f <= 8 e* + 55
  u cr``; the divisions by cr cancel against the factor ``v s = cr`` that
  multiplies f, so a nearly grey pixel is not ill-conditioned.  The three
  roundings of ``v (1 - s f)`` are ``3 u v``, ``1 - f`` one more ``u cr``.
  Every channel: ``12 e* + 5 u v + 57 u cr``.
* coordinate: ``g = bx (m0 / hw) + by (m1 / hw) + m2 / hw``: per term a division
  and a product, two sums: ``4 u A`` with ``A = |bx m0 / hw| + |by m1 / hw|``;
  ``(g + 1) W - 1`` over 2: three more roundings:
  ``delta = u (4 A W + 2 (A + 1) W + (A + 1) W + 1) / 2``.
* bilinear: weight product, value product, three sums, the same for the mask,
  their product: ``10 u sum w |J|``.

All of it is first order; ``SECOND_ORDER`` = 1.01 multiplies the total for the
products of (1 + u) factors and ``4 delta^2`` is added for the curvature of
``S M`` (bilinear value times bilinear mask) within delta.

Largest share of two-candidate label pixels found in any case: 0 % -- delta is
about 1e-5 of a pixel, the rotated cases' coordinates are generic, and at 0, 90
(equal parity) and 180 degrees they are integers, half a pixel from the tie.
The systematic ties (a quarter turn at unequal parity, the diagonal of a 45
degree turn on even sizes) run with ``label=None``.  The builders assert
<= 1 % (``MAX_LABEL_SHARE``); tests/test_augment_reference_cpu.py prints what a
run finds.
"""
from __future__ import annotations

import functools
import itertools
import math

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SECOND_ORDER = 1.01
MAX_LABEL_SHARE = 0.01
LAUNCH = 16                     # AUG_MAX_BATCH: images per launch
GREY = (0.2989, 0.587, 0.114)
WORST = {}


class Mismatch(AssertionError):
    pass


def f32(x) -> float:
    """the float32 value of x, as a Python float"""
    return float(F32(x))


# ---------------------------------------------------------------------------
# ColorJitter of pixels [N,3], value and error bound
# ---------------------------------------------------------------------------
def _clamp(x, mutant):
    if mutant == "nan_clamped":
        return np.fmin(np.fmax(x, 0.0), 1.0)
    return np.clip(x, 0.0, 1.0)         # hands a NaN on


def _blend(a, ea, b, eb, f, mutant, clamp=True):
    v = f * a + (1.0 - f) * b
    e = abs(f) * ea + abs(1.0 - f) * eb + U * (2 * np.abs(f * a) + 3 * np.abs((1.0 - f) * b))
    if clamp:
        # an infinite blend is clamped to exactly 0 or 1 by every evaluation
        v, e = _clamp(v, mutant), np.where(np.isinf(v), 0.0, e)
    return v, e


def grey(v, e, mutant=None):
    """grey level of pixels [...,3] and its error bound"""
    c = (0.299,) + GREY[1:] if mutant == "grey_0299" else GREY
    terms = [c[k] * v[..., k] for k in range(3)]
    l = terms[0] + terms[1] + terms[2]
    el = sum(c[k] * e[..., k] for k in range(3)) + 4 * U * sum(np.abs(t) for t in terms)
    return l, el


def _hue(v, e, hue, mutant):
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    if mutant == "nan_clamped":
        maxc, minc = np.fmax(r, np.fmax(g, b)), np.fmin(r, np.fmin(g, b))
    else:
        maxc, minc = np.max(v, -1), np.min(v, -1)
    eqc = maxc == minc
    if mutant == "no_eqc_guard":
        eqc = np.zeros_like(eqc)
    cr = maxc - minc
    s = cr / np.where(eqc, 1.0, maxc)
    div = np.where(eqc, 1.0, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    is_r, is_g = maxc == r, maxc == g
    if mutant == "tie_green_first":
        # green claims a tie with red (the `maxc != r` is gone), red still does
        green = is_g
    elif mutant == "tie_green_consistent":
        green, is_r = is_g, is_r & ~is_g
    else:
        green = is_g & ~is_r
    nan = np.isnan(maxc)
    hr = np.where(is_r, bc - gc, 0.0)
    hg = np.where(green, 2.0 + rc - bc, 0.0)
    hb = np.where(~is_g & ~is_r, 4.0 + gc - rc, 0.0)
    h = hr + hg + hb
    h = np.where(nan, np.nan, h)
    h = np.fmod(h / 6.0 + 1.0, 1.0)
    h = h + hue
    if mutant not in ("hue_not_wrapped", "hue_unwrapped_mod6"):
        h = h - np.floor(h)                  # python-style % 1.0
    h6 = h * 6.0
    fi = np.floor(h6)
    f = h6 - fi
    if mutant == "sector_rounded":
        fi = np.rint(h6)
    p = _clamp(maxc * (1.0 - s), mutant)
    q = _clamp(maxc * (1.0 - s * f), mutant)
    t = _clamp(maxc * (1.0 - s * (1.0 - f)), mutant)
    fin = np.where(np.isfinite(fi), fi, 4.0)     # torch on x86: int32(NaN) % 6 == 4
    if mutant == "hue_not_wrapped":
        # no `% 1.0`, and the sector goes to a switch with no `% 6`: -1 and 6
        # both land in its default, which is sector 5
        i = np.where((fin < 0) | (fin > 5), 5, fin).astype(np.int64)
    else:
        i = np.mod(fin, 6.0).astype(np.int64)
    vv = maxc
    tab = np.stack([np.stack(x, -1) for x in ((vv, t, p), (q, vv, p), (p, vv, t),
                                               (p, q, vv), (t, p, vv), (vv, p, q))], 0)
    out = np.take_along_axis(tab, i[None, ..., None], 0)[0]
    es = np.max(e, -1)
    eo = 12 * es + 5 * U * np.abs(maxc) + 57 * U * np.abs(cr)
    return out, np.repeat(eo[..., None], 3, -1)


def jitter(px, p, mean=0.0, e_mean=0.0, stop_at_contrast=False, mutant=None):
    """The ops of ``p['order']`` on pixels [...,3] -> (value, error bound), both
    float64.  With ``stop_at_contrast`` the pixels are returned as they enter
    the contrast op."""
    v = np.asarray(px, F64)
    e = np.zeros_like(v)
    bf, cf, sf, hf = (f32(p[k]) for k in ("brightness", "contrast", "saturation", "hue"))
    with np.errstate(all="ignore"):
        for op in p["order"]:
            if op == 0:
                v, e = _blend(v, e, 0.0, 0.0, bf, mutant, clamp=mutant != "no_clamp")
            elif op == 1:
                if stop_at_contrast:
                    return v, e
                v, e = _blend(v, e, mean, e_mean, cf, mutant)
            elif op == 2:
                l, el = grey(v, e, mutant)
                v, e = _blend(v, e, l[..., None], el[..., None], sf, mutant)
            elif op == 3:
                v, e = _hue(v, e, hf, mutant)
    return v, e


def contrast_mean(img, p, out_hw=None, mutant=None):
    """mean grey level of ``img`` [3,H,W] as it enters the contrast op, and the
    bound of a float32 evaluation's error in it"""
    px = np.asarray(img, F64).reshape(3, -1).T
    P = px.shape[0]
    with np.errstate(all="ignore"):
        if mutant == "mean_of_input":
            v, e = px, np.zeros_like(px)
        else:
            v, e = jitter(px, p, stop_at_contrast=True, mutant=mutant)
        l, el = grey(v, e, mutant)
        if mutant == "mean_tail_lost":
            mean = l[:1024 * (P // 1024)].sum() / P
        elif mutant == "mean_div_ohow":
            mean = l.sum() / (out_hw[0] * out_hw[1])
        else:
            mean = l.sum() / P
        e_mean = el.sum() / P + (2 + math.ceil(math.log2(P)) if P > 1 else 2) * U * np.abs(l).sum() / P
    return float(mean), float(e_mean)


# ---------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------
def rotation_matrix(angle_deg):
    """inverse rotation, row-major 2x3: cos / sin in double, rounded to float32"""
    rot = -f32(angle_deg) * math.pi / 180.0
    ca, sa = math.cos(rot), math.sin(rot)
    return np.array([ca, sa, 0.0, -sa, ca, 0.0], F32).astype(F64)


def source_coords(H, W, oh, ow, p, mutant=None):
    """(ix, iy, dx, dy) [oh,ow]: the source coordinate of every output pixel and
    the bound of a float32 evaluation's error in it"""
    m = rotation_matrix(p["angle_deg"])
    if mutant == "rotation_sign":
        m[1], m[3] = -m[1], -m[3]
    oy, ox = np.mgrid[0:oh, 0:ow].astype(F64)
    ci, cj = int(p.get("crop_i", 0)), int(p.get("crop_j", 0))
    if mutant == "crop_swapped":
        ci, cj = cj, ci
    if mutant == "flip_before_crop":
        rx = (W - 1 - (cj + ox)) if p["flip"] else cj + ox
    elif mutant == "flip_about_w":
        rx = cj + ((W - 1 - ox) if p["flip"] else ox)
    else:
        rx = cj + ((ow - 1 - ox) if p["flip"] else ox)
    ry = ci + oy
    half = 0.0 if mutant == "no_half" else 0.5
    bx, by = -W * 0.5 + half + rx, -H * 0.5 + half + ry
    hw, hh = 0.5 * W, 0.5 * H

    def axis(c0, c1, c2, n, h):
        t0, t1 = bx * (c0 / h), by * (c1 / h)
        g = t0 + t1 + c2 / h
        A = np.abs(t0) + np.abs(t1)
        d = U * (4 * A * n + 2 * (A + 1) * n + (A + 1) * n + 1) / 2
        return ((g + 1.0) * n - 1.0) / 2.0, d

    ix, dx = axis(m[0], m[1], m[2], W, hw)
    iy, dy = axis(m[3], m[4], m[5], H, hh)
    return ix, iy, dx, dy


def _cell(J, x0, y0, ix, iy, mutant=None):
    """bilinear value times mask in the cell whose corner is (x0, y0), and its
    partial derivatives, from the float64 corner values; zero padding"""
    H, W = J.shape[:2]
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1.0 - wx1, 1.0 - wy1
    if mutant == "weights_swapped_x":
        wx0, wx1 = wx1, wx0
    v, m = {}, {}
    for dy in (0, 1):
        for dx in (0, 1):
            xx, yy = (x0 + dx).astype(np.int64), (y0 + dy).astype(np.int64)
            inb = (xx >= 0) & (yy >= 0) & (xx < W) & (yy < H)
            val = J[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
            v[dx, dy] = np.where(inb[..., None], val, 0.0)
            m[dx, dy] = inb.astype(F64)
    w = {(0, 0): wx0 * wy0, (1, 0): wx1 * wy0, (0, 1): wx0 * wy1, (1, 1): wx1 * wy1}
    with np.errstate(all="ignore"):
        S = sum(w[k][..., None] * v[k] for k in w)
        Sabs = sum(np.abs(w[k])[..., None] * np.abs(v[k]) for k in w)
        M = sum(w[k] * m[k] for k in w)[..., None]
        Sx = wy0[..., None] * (v[1, 0] - v[0, 0]) + wy1[..., None] * (v[1, 1] - v[0, 1])
        Sy = wx0[..., None] * (v[0, 1] - v[0, 0]) + wx1[..., None] * (v[1, 1] - v[1, 0])
        Mx = (wy0 * (m[1, 0] - m[0, 0]) + wy1 * (m[1, 1] - m[0, 1]))[..., None]
        My = (wx0 * (m[0, 1] - m[0, 0]) + wx1 * (m[1, 1] - m[1, 0]))[..., None]
        if mutant == "no_mask":
            return S, Sabs, np.abs(Sx), np.abs(Sy), w, v, m
        return S * M, Sabs * M, np.abs(Sx * M + S * Mx), np.abs(Sy * M + S * My), w, v, m


def bilinear(J, EJ, ix, iy, dx, dy, mutant=None):
    """(value, bound) [oh,ow,3] of the bilinear sample of the jittered image
    ``J`` [H,W,3] (error bound ``EJ``) at (ix, iy) +- (dx, dy), zero padding,
    times the sampled ones-mask"""
    x0, y0 = np.floor(ix), np.floor(iy)
    out, Sabs, gx, gy, w, v, m = _cell(J, x0, y0, ix, iy, mutant)
    # corner errors through the weights (EJ sampled like J, mask included)
    Eo = _cell(EJ, x0, y0, ix, iy)[0]
    # within delta of an integer: the larger gradient of the adjoining cells
    for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)):
        x1 = np.floor(ix + sx * dx) if sx else x0
        y1 = np.floor(iy + sy * dy) if sy else y0
        near = (x1 != x0) | (y1 != y0)
        if near.any():
            _, _, g2x, g2y, _, _, _ = _cell(J, x1, y1, ix, iy)
            Eo2 = _cell(EJ, x1, y1, ix, iy)[0]
            n3 = near[..., None]
            gx, gy = np.where(n3, np.fmax(gx, g2x), gx), np.where(n3, np.fmax(gy, g2y), gy)
            Eo = np.where(n3, np.fmax(Eo, Eo2), Eo)
    with np.errstate(all="ignore"):
        # nothing but zeros in every cell within delta (out of frame, or black
        # with no error): the value is an exact 0 and the bound is 0
        live = (gx + gy + Sabs + Eo) != 0
        bound = Eo + dx[..., None] * gx + dy[..., None] * gy + 10 * U * Sabs \
            + np.where(live, 4 * (dx * dx + dy * dy)[..., None], 0.0)
        bound = SECOND_ORDER * bound
    return out, bound


def nearest_label(label, ix, iy, dx=None, dy=None, mutant=None):
    """labels [oh,ow] by round-half-to-even, -1 out of frame; with (dx, dy) also
    the candidates [oh,ow,4] a float32 coordinate within them may land on"""
    H, W = label.shape
    fill = 0 if mutant == "label_fill_0" else -1

    def pick(xn, yn):
        xn, yn = xn.astype(np.int64), yn.astype(np.int64)
        inb = (xn >= 0) & (yn >= 0) & (xn < W) & (yn < H)
        return np.where(inb, label[np.clip(yn, 0, H - 1), np.clip(xn, 0, W - 1)], fill)

    if mutant == "label_floor":
        rnd = np.floor
    elif mutant == "label_half_away":
        rnd = lambda x: np.sign(x) * np.floor(np.abs(x) + 0.5)
    else:
        rnd = np.rint
    lab = pick(rnd(ix), rnd(iy))
    if dx is None:
        return lab
    xs, ys = (np.rint(ix - dx), np.rint(ix + dx)), (np.rint(iy - dy), np.rint(iy + dy))
    cands = np.stack([pick(x, y) for x in xs for y in ys], -1)
    two = (xs[0] != xs[1]) | (ys[0] != ys[1])
    return lab, cands, two


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
class Case:
    def __init__(self, name, img, label, params, out_size=None, pinned=False):
        self.name = name
        self.img = np.ascontiguousarray(img, F32)
        self.label = None if label is None else np.ascontiguousarray(label, np.int64)
        self.params = params
        self.B, _, self.H, self.W = self.img.shape
        self.out_size = (self.H, self.W) if out_size is None else tuple(out_size)
        assert len(params) == self.B
        self.share = self._label_share()
        assert self.share <= MAX_LABEL_SHARE, (name, self.share)
        if pinned:
            # 0 * NaN is where the image path is NOT continuous: a case with a
            # NaN among finite pixels keeps every coordinate clear of the cell edges
            for p in params:
                ix, iy, dx, dy = source_coords(self.H, self.W, *self.out_size, p)
                assert (np.floor(ix - dx) == np.floor(ix + dx)).all(), name
                assert (np.floor(iy - dy) == np.floor(iy + dy)).all(), name

    def _label_share(self):
        if self.label is None or self.B == 0:
            return 0.0
        worst = 0.0
        for p in self.params:
            ix, iy, dx, dy = source_coords(self.H, self.W, *self.out_size, p)
            two = nearest_label(self.label[0], ix, iy, dx, dy)[2]
            worst = max(worst, float(two.mean()))
        return worst

    def without_label(self):
        return Case(self.name, self.img, None, self.params, self.out_size)


class Ref:
    def __init__(self, img, bound, label, cands):
        self.img, self.bound, self.label, self.cands = img, bound, label, cands


def evaluate(c, mutant=None):
    """-> Ref: the float64 image [B,3,oh,ow] with its bounds and the labels
    [B,oh,ow] with their candidates.  ``mutant`` names a deliberate mistake."""
    oh, ow = c.out_size
    img_o = np.zeros((c.B, 3, oh, ow), F64)
    bnd_o = np.zeros_like(img_o)
    lab_o = None if c.label is None else np.zeros((c.B, oh, ow), np.int64)
    cand_o = None if c.label is None else np.zeros((c.B, oh, ow, 4), np.int64)
    for b in range(c.B):
        slot = b % LAUNCH
        p = c.params[slot if mutant == "params_first_launch" else b]
        src = slot if mutant == "image_no_b0" else b
        im = c.img[src]
        mean, e_mean = contrast_mean(c.img[slot] if mutant == "mean_wrong_b0" else im, p,
                                     c.out_size, mutant)
        J, EJ = jitter(np.moveaxis(im, 0, -1), p, mean, e_mean, mutant=mutant)
        ix, iy, dx, dy = source_coords(c.H, c.W, oh, ow, p, mutant)
        out, bound = bilinear(J, EJ, ix, iy, dx, dy, mutant)
        img_o[b], bnd_o[b] = np.moveaxis(out, -1, 0), np.moveaxis(bound, -1, 0)
        if c.label is not None:
            lab_o[b], cand_o[b], _ = nearest_label(c.label[src], ix, iy, dx, dy, mutant)
    return Ref(img_o, bnd_o, lab_o, cand_o)


@functools.lru_cache(maxsize=None)
def reference(name):
    return evaluate(build_case(name))


def compare(got_img, got_label, ref, what, name=""):
    """Every image value within its bound of the reference (identical where the
    bound is not finite: NaN for NaN, the clamped 1 for inf), every label one of
    its candidates.  Records the worst err / bound under ``what``."""
    got = np.asarray(got_img, F64)
    if got.shape != ref.img.shape:
        raise Mismatch(f"{what} {name}: image shape {got.shape} for {ref.img.shape}")
    exact = ~np.isfinite(ref.bound) | ~np.isfinite(ref.img)
    same = (got == ref.img) | (np.isnan(got) & np.isnan(ref.img))
    if not same[exact].all():
        k = np.argwhere(exact & ~same)[0]
        raise Mismatch(f"{what} {name}: at {tuple(k)} got {got[tuple(k)]!r}, "
                       f"the reference has {ref.img[tuple(k)]!r} ({int((exact & ~same).sum())} such)")
    with np.errstate(all="ignore"):
        err = np.where(exact, 0.0, np.abs(got - ref.img))
        err = np.where(np.isnan(err), np.inf, err)
        ratio = np.where(err == 0, 0.0, err / np.where(exact, 1.0, ref.bound))
    worst = float(ratio.max()) if ratio.size else 0.0
    WORST[what + " image"] = max(WORST.get(what + " image", 0.0), worst)
    if not worst <= 1.0:
        k = tuple(np.unravel_index(np.argmax(ratio), ratio.shape))
        raise Mismatch(f"{what} {name}: image at {k}: got {got[k]!r}, reference {ref.img[k]!r}, "
                       f"err {err[k]:.3e} > bound {ref.bound[k]:.3e} ({int((ratio > 1).sum())} outside)")
    if ref.label is None:
        if got_label is not None:
            raise Mismatch(f"{what} {name}: a label came back where none went in")
        return worst
    gl = np.asarray(got_label)
    if gl.shape != ref.label.shape:
        raise Mismatch(f"{what} {name}: label shape {gl.shape} for {ref.label.shape}")
    ok = (gl[..., None] == ref.cands).any(-1)
    if not ok.all():
        k = tuple(np.argwhere(~ok)[0])
        raise Mismatch(f"{what} {name}: label at {k}: got {gl[k]}, candidates "
                       f"{sorted(set(ref.cands[k].tolist()))} ({int((~ok).sum())} wrong)")
    return worst


# ---- builders --------------------------------------------------------------
def _noise(rng, B, H, W):
    return rng.random((B, 3, H, W), dtype=F32)


def _labels(rng, B, H, W):
    return rng.integers(-1, 40, (B, H, W))


def _param(order=(0, 1, 2, 3), b=1.0, c=1.0, s=1.0, h=0.0, angle=0.0, flip=False, crop=(0, 0)):
    return dict(order=list(order), brightness=b, contrast=c, saturation=s, hue=h,
                angle_deg=angle, flip=bool(flip), crop_i=int(crop[0]), crop_j=int(crop[1]))


def _random_param(rng, H, W, oh, ow, rotate=True):
    return _param(rng.permutation(4).tolist(), *rng.uniform(0.7, 1.3, 3), rng.uniform(-0.05, 0.05),
                  rng.uniform(-10, 10) if rotate else 0.0, rng.random() < 0.5,
                  (rng.integers(0, H - oh + 1), rng.integers(0, W - ow + 1)))


def hsv_pixel(h, s, v):
    """an rgb pixel of hue h (float64 hsv -> rgb, then rounded to float32)"""
    h6 = (h % 1.0) * 6.0
    i, f = int(math.floor(h6)) % 6, h6 - math.floor(h6)
    p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
    return [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)][i]


def pixel_table():
    """The 8 x 16 table image [3,8,16] of hand-placed pixels (the rest noise) and
    the names of its leading entries."""
    up = float(np.nextafter(F32(0.5), F32(1)))
    eps = 1e-6
    px = [("black", (0, 0, 0)), ("white", (1, 1, 1)), ("grey", (0.5, 0.5, 0.5)),
          ("grey_r_ulp", (up, 0.5, 0.5)), ("grey_g_ulp", (0.5, up, 0.5)), ("grey_b_ulp", (0.5, 0.5, up)),
          ("tie_rg", (0.75, 0.75, 0.25)), ("tie_rb", (0.75, 0.25, 0.75)), ("tie_gb", (0.25, 0.75, 0.75)),
          ("ones", (1, 1, 1)), ("minc0", (0.625, 0.375, 0.0)), ("minc0_b", (0.0, 0.25, 0.875))]
    px += [(f"primary{k}", hsv_pixel(k / 6.0, 1.0, 1.0)) for k in range(6)]
    px += [(f"dim_primary{k}", hsv_pixel(k / 6.0, 0.5, 0.5)) for k in range(6)]
    px += [("clamp_hi", (0.9, 0.8, 0.95)), ("clamp_lo", (0.05, 0.0, 0.1)), ("clamp_mixed", (1.0, 0.0, 0.85))]
    for hue in (0.05, -0.05, 0.5, -0.5):
        # h + hue lands on 0 (= 1) and on every sector boundary, from both sides
        for k in range(6):
            for side in (-eps, 0.0, eps):
                px.append((f"land{k}_{hue}_{side}", hsv_pixel(k / 6.0 - hue + side, 0.75, 0.875)))
    assert len(px) <= 128, len(px)
    rng = np.random.default_rng(11)
    tab = rng.random((128, 3), dtype=F32)
    tab[:len(px)] = np.array([v for _, v in px], F64).astype(F32)
    return np.ascontiguousarray(tab.T.reshape(3, 8, 16)), [n for n, _ in px]


def _pixels_case(name):
    tab, _ = pixel_table()
    params = []
    mild = dict(b=1.3, c=0.7, s=1.3, h=0.05)
    names = "bcs"
    for op in range(3):            # brightness / contrast / saturation first, at 0, 1, 2
        order = [op] + [k for k in range(4) if k != op]
        for level in (0.0, 1.0, 2.0):
            params.append(_param(order, **{**mild, names[op]: level}))
    for hue in (-0.5, -0.05, 0.0, 0.05, 0.5):       # hue first
        params.append(_param([3, 0, 1, 2], **{**mild, "h": hue}))
    for level, hue in ((0.0, 0.5), (1.0, -0.5), (2.0, 0.05)):   # every factor at once
        params.append(_param([3, 2, 1, 0], level, level, level, hue))
    B = len(params)
    rng = np.random.default_rng(12)
    return Case(name, np.repeat(tab[None], B, 0), _labels(rng, B, 8, 16), params)


def _orders_case(name):
    rng = np.random.default_rng(21)
    perms = list(itertools.permutations(range(4)))
    ends = lambda k, lo, hi: hi if k else lo
    params = [_param(o, ends(k & 1, 0.7, 1.3), ends((k >> 1) & 1 ^ (k & 1), 0.7, 1.3),
                     ends((k >> 2) & 1, 0.7, 1.3), ends((k // 3) & 1, -0.05, 0.05))
              for k, o in enumerate(perms)]
    return Case(name, _noise(rng, 24, 24, 40), _labels(rng, 24, 24, 40), params)


MEAN_SIZES = [(1, 1), (1, 255), (3, 343), (17, 61), (64, 65)]
MEAN_VARIANTS = {"bc": _param([0, 1, 2, 3], 1.3, 1.3, 0.7, 0.05),
                 "hs": _param([3, 2, 1, 0], 1.3, 1.3, 0.7, 0.05),
                 "outlier": _param([0, 1, 2, 3], 1.3, 1.3, 0.7, 0.05)}


def _mean_case(name):
    _, size, variant = name.split("_")
    H, W = (int(v) for v in size.split("x"))
    rng = np.random.default_rng(31 + H * W)
    img = _noise(rng, 1, H, W)
    if variant == "outlier":
        img[:] = np.array([0.25, 0.5, 0.125], F32)[None, :, None, None]
        img[0, :, H - 1, W - 1] = (1.0, 0.875, 1.0)
    oh, ow = max(1, H - 1 - H // 8), max(1, W - 2 - W // 8)
    p = dict(MEAN_VARIANTS[variant], crop_i=min(1, H - oh), crop_j=min(2, W - ow))
    return Case(name, img, _labels(rng, 1, H, W), [p], (oh, ow))


ROT_ANGLES = [0.0, 1e-3, 7.3, -10.0, 45.0, 90.0, -90.0, 180.0]
ROT_SIZES = [(17, 23), (16, 23), (1, 37), (37, 1), (24, 40)]


def rotation_has_label(H, W, angle):
    """Quarter turns put every coordinate on a half-integer when H and W differ
    in parity, 45 degrees puts a diagonal there when both are even: image only."""
    if abs(angle) == 90.0:
        return (H - W) % 2 == 0
    if abs(angle) == 45.0:
        return H % 2 == 1 or W % 2 == 1
    return True


def _rotation_case(name):
    _, size, ang = name.split("_")
    H, W = (int(v) for v in size.split("x"))
    angle = float(ang)
    rng = np.random.default_rng([41, H, W, int(angle * 1000) + 10 ** 6])
    p = _random_param(rng, H, W, H, W)
    p["angle_deg"] = angle
    lab = _labels(rng, 1, H, W) if rotation_has_label(H, W, angle) else None
    return Case(name, _noise(rng, 1, H, W), lab, [p])


def _crop_flip_case(name):
    H, W = 19, 27
    oh, ow = (7, 1) if name.endswith("ow1") else (7, 11)
    rng = np.random.default_rng(51)
    params = []
    for crop in ((0, 0), (H - oh, W - ow), (3, 8)):
        for flip in (False, True):
            for angle in (0.0, 7.3):
                p = _random_param(rng, H, W, oh, ow)
                p.update(angle_deg=angle, flip=flip, crop_i=crop[0], crop_j=crop[1])
                params.append(p)
    B = len(params)
    lab = None if name.endswith("nolabel") else _labels(rng, B, H, W)
    return Case(name, _noise(rng, B, H, W), lab, params, (oh, ow))


def _batch_case(name):
    B = int(name[len("batch"):])
    rng = np.random.default_rng(61)
    H, W, oh, ow = 9, 13, 7, 11
    params = [_random_param(rng, H, W, oh, ow) for _ in range(B)]
    return Case(name, _noise(rng, B, H, W), _labels(rng, B, H, W), params, (oh, ow))


NONFINITE = {
    # name: (bad value, params)
    "nonfinite_nan_contrast_first": (np.nan, _param([1, 0, 2, 3], 1.3, 1.3, 0.7, 0.05)),
    "nonfinite_nan_contrast_last": (np.nan, _param([0, 2, 3, 1], 1.3, 0.7, 0.7, 0.05)),
    "nonfinite_nan_hue_first": (np.nan, _param([3, 0, 2, 1], 1.3, 1.3, 0.7, 0.05)),
    "nonfinite_nan_rotated": (np.nan, _param([0, 2, 3, 1], 1.3, 1.3, 0.7, 0.05, angle=45.0)),
    # inf into the mean: contrast < 1 blends every pixel to +inf, clamped to 1;
    # the later ops keep an all-white image at exactly 1
    "nonfinite_inf_contrast_first_white": (np.inf, _param([1, 0, 2, 3], 1.3, 0.7, 1.3, 0.05)),
    # contrast > 1: every finite pixel goes to -inf and is clamped to 0, the
    # inf pixel is inf - inf: one NaN in a black image, rotated so that no
    # coordinate sits on a cell edge (Case(pinned=True))
    "nonfinite_inf_contrast_first": (np.inf, _param([1, 0, 2, 3], 1.3, 1.3, 0.7, 0.05, angle=7.3)),
    # brightness clamps the inf to 1 before anything sees it: a white pixel
    "nonfinite_inf_contrast_last": (np.inf, _param([0, 2, 3, 1], 1.3, 1.3, 0.7, 0.05)),
    # the hue op makes inf / inf of it
    "nonfinite_inf_hue_first": (np.inf, _param([3, 0, 2, 1], 1.3, 1.3, 0.7, 0.05)),
}


def _nonfinite_case(name):
    bad, p = NONFINITE[name]
    rng = np.random.default_rng(71)
    pinned = name == "nonfinite_inf_contrast_first"
    H, W = (8, 12) if pinned else (9, 13)     # odd sizes put the centre pixel on a cell corner
    img = _noise(rng, 2, H, W)
    img[0, 1, 4, 6] = bad            # one channel of one pixel; image 1 stays clean
    return Case(name, img, _labels(rng, 2, H, W), [p, dict(p, flip=True)],
                pinned=pinned)


FAMILIES = {
    "orders": (_orders_case, ["orders"]),
    "pixels": (_pixels_case, ["pixels"]),
    "mean": (_mean_case, [f"mean_{H}x{W}_{v}" for H, W in MEAN_SIZES for v in MEAN_VARIANTS]),
    "rotation": (_rotation_case, [f"rotation_{H}x{W}_{a:g}" for H, W in ROT_SIZES for a in ROT_ANGLES]),
    "crop_flip": (_crop_flip_case, ["crop_flip", "crop_flip_ow1", "crop_flip_nolabel"]),
    "batch": (_batch_case, ["batch1", "batch16", "batch17", "batch33"]),
    "nonfinite": (_nonfinite_case, list(NONFINITE)),
}


def case_specs(family=None):
    """case names, of one family or of all"""
    fams = [family] if family else list(FAMILIES)
    return [n for f in fams for n in FAMILIES[f][1]]


def family_of(name):
    for f, (_, names) in FAMILIES.items():
        if name in names:
            return f
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def build_case(name):
    return FAMILIES[family_of(name)][0](name)


# deliberate mistakes `evaluate` can make; tests/test_augment_reference_cpu.py
# names the case that rejects each (KILLED_BY)
MUTANTS = [
    "grey_0299", "mean_of_input", "mean_tail_lost", "mean_div_ohow", "mean_wrong_b0",
    "params_first_launch", "image_no_b0", "no_clamp", "hue_not_wrapped", "sector_rounded",
    "tie_green_first", "no_eqc_guard", "nan_clamped", "flip_about_w", "flip_before_crop",
    "crop_swapped", "rotation_sign", "no_half", "no_mask", "label_fill_0", "label_floor",
    "weights_swapped_x",
]
# other ways to write it that are the SAME function (test_what_the_cases_cannot_see)
EQUIVALENT = ["label_half_away", "tie_green_consistent", "hue_unwrapped_mod6"]
