"""``ucsa_augment`` (``k_aug_grey_sum`` + ``k_aug_apply``) against the float64
reference of tests/augment_numpy.py, value by value, within bounds derived
there from counting rounding steps: no image value is exempt and there is no
flat tolerance; a label must be one of the reference's candidates, of which
there is exactly one wherever the coordinate is clear of the half-way lines.
tests/test_augment_reference_cpu.py holds the reference against the oracle and
names, per deliberate mistake, the case here that rejects it (``KILLED_BY``).

Worst err / bound per case family, as printed at the end of a run on an
MI355X: docs/DESIGN_NOTEBOOK.md, section AR."""
import numpy as np
import pytest
import torch

from tests import augment_numpy as an

pytestmark = pytest.mark.gpu
SENTINEL_F, SENTINEL_L = -7.25, -77


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    yield _ops
    if an.WORST:
        print("\nworst err / bound per case family and output:")
        for k in sorted(an.WORST):
            print(f"  {k}: {an.WORST[k]:.3f}")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    """a faulted device ends the module: no later test launches on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _lib():
    from ucsa_neural_rendering_amd import _lib as L
    return L


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


class _Args:
    """pointers for a C ABI call; the device copies they point to stay alive
    until the caller has synchronised"""

    def __init__(self, ops):
        self.ptr, self.keep = ops._ptr, []

    def __call__(self, a, dtype=torch.float32):
        t = a if (a is None or torch.is_tensor(a)) else _dev(a, dtype)
        self.keep.append(t)
        return self.ptr(t)


def _bits(t):
    return np.atleast_1d(t.detach().cpu().contiguous().numpy()).view(np.uint8).tobytes()


def _run(ops, c, label=True):
    lab = _dev(c.label, torch.int64) if label else None
    out, out_l = ops.augment(_dev(c.img), lab, c.params, c.out_size)
    torch.cuda.synchronize()
    return out, out_l


def _check(ops, name):
    """the case through ops.augment against the reference; a second call and a
    call without the label give the same image bytes"""
    c, ref = an.build_case(name), an.reference(name)
    out, out_l = _run(ops, c)
    assert (out_l is None) == (c.label is None)
    an.compare(out.cpu().numpy(), None if out_l is None else out_l.cpu().numpy(), ref,
               f"augment {an.family_of(name)}", name)
    again, again_l = _run(ops, c)
    assert _bits(again) == _bits(out), "second call differs"
    if c.label is not None:
        assert _bits(again_l) == _bits(out_l), "second call differs in the label"
        bare, none = _run(ops, c, label=False)
        assert none is None and _bits(bare) == _bits(out), "label=None changes the image"


@pytest.mark.parametrize("name", an.case_specs("orders"))
def test_orders(ops, name):
    """all 24 op orders in two launches: the mean grey level is that of the image
    as it enters the contrast op"""
    _check(ops, name)


@pytest.mark.parametrize("name", an.case_specs("pixels"))
def test_pixels(ops, name):
    """the table of grey, black, white, tied, primary, clamping and sector-edge
    pixels with each op first, factors 0 / 1 / 2 and hue out to +-0.5"""
    _check(ops, name)


@pytest.mark.parametrize("name", an.case_specs("mean"))
def test_mean(ops, name):
    """P = 1, P < 256, tails that are no multiple of 1024, oh * ow != H * W; the
    image gives the same bytes alone and as the last of B = 17 (slot 0 of the
    second launch, after the workspace has held 16 other images' sums)"""
    _check(ops, name)
    c = an.build_case(name)
    rng = np.random.default_rng(7)
    oh, ow = c.out_size
    others = [an._random_param(rng, c.H, c.W, oh, ow) for _ in range(16)]
    img = np.concatenate([an._noise(rng, 16, c.H, c.W), c.img], 0)
    alone, _ = _run(ops, c, label=False)
    out, _ = ops.augment(_dev(img), None, others + c.params, c.out_size)
    torch.cuda.synchronize()
    assert _bits(out[16]) == _bits(alone[0])


@pytest.mark.parametrize("name", an.case_specs("rotation"))
def test_rotation(ops, name):
    """0, tiny, generic, 45, quarter and half turns on odd, even, 1 x N and N x 1
    images; rows wholly out of frame are exact zeros and -1"""
    _check(ops, name)


@pytest.mark.parametrize("name", an.case_specs("crop_flip"))
def test_crop_flip(ops, name):
    """corner and interior crops, flipped and not, straight and rotated"""
    _check(ops, name)


@pytest.mark.parametrize("name", an.case_specs("batch"))
def test_batch(ops, name):
    """B = 1, 16, 17, 33: one, one full, two and three launches, every image,
    label and parameter set distinct"""
    _check(ops, name)


@pytest.mark.parametrize("name", an.case_specs("nonfinite"))
def test_nonfinite(ops, name):
    """a NaN or inf pixel propagates as in torch: through the clamps, the hue
    op's max / min and the contrast mean; the clean second image stays finite"""
    _check(ops, name)
    out, _ = _run(ops, an.build_case(name))
    assert bool(torch.isfinite(out[1]).all())


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def _abi(ops, c, order0=None, crop0=None, out_size=None, label=True, out_label=True, B=None):
    """ucsa_augment on caller-owned outputs carved from larger allocations with
    sentinel words around them -> rc, out_img, out_label, intact()"""
    L = _lib()
    p = _Args(ops)
    oh, ow = out_size or c.out_size
    B = c.B if B is None else B
    arr = (L.AugParams * max(B, 1))()
    for k, q in enumerate(c.params[:B]):
        arr[k].order[:] = q["order"] if (k or order0 is None) else order0
        arr[k].brightness, arr[k].contrast = q["brightness"], q["contrast"]
        arr[k].saturation, arr[k].hue, arr[k].angle_deg = q["saturation"], q["hue"], q["angle_deg"]
        arr[k].flip = int(q["flip"])
        arr[k].crop_i, arr[k].crop_j = (q["crop_i"], q["crop_j"]) if (k or crop0 is None) else crop0
    n_img, n_lab = c.B * 3 * oh * ow, c.B * oh * ow
    big_f = torch.full((n_img + 24,), SENTINEL_F, device="cuda")
    big_l = torch.full((n_lab + 11,), SENTINEL_L, dtype=torch.int64, device="cuda")
    out, out_l = big_f[13:13 + n_img], big_l[5:5 + n_lab]
    ws = torch.empty(int(L.lib().ucsa_augment_workspace_bytes(c.B, c.H, c.W)), dtype=torch.uint8, device="cuda")
    rc = L.lib().ucsa_augment(p(c.img), p(c.label, torch.int64) if label else None, B, c.H, c.W, arr, oh, ow,
                              p(out), p(out_l) if out_label else None, p(ws), ops._stream())
    torch.cuda.synchronize()

    def intact(everything=False):
        f, l = big_f.cpu().numpy(), big_l.cpu().numpy()
        if everything:
            return bool((f == SENTINEL_F).all() and (l == SENTINEL_L).all())
        return bool((f[:13] == SENTINEL_F).all() and (f[13 + n_img:] == SENTINEL_F).all()
                    and (l[:5] == SENTINEL_L).all() and (l[5 + n_lab:] == SENTINEL_L).all())

    return rc, out.view(c.B, 3, oh, ow), out_l.view(c.B, oh, ow), intact


def test_c_abi_writes_its_outputs_and_nothing_else(ops):
    """B = 17, oh * ow = 7 * 11: the last block of each image is partly idle and
    the second launch starts at b0 = 16"""
    c, ref = an.build_case("batch17"), an.reference("batch17")
    assert c.B == 17 and c.out_size == (7, 11)
    rc, out, out_l, intact = _abi(ops, c)
    assert rc == 0
    an.compare(out.cpu().numpy(), out_l.cpu().numpy(), ref, "augment c abi", c.name)
    assert intact(), "a sentinel next to the outputs was overwritten"
    assert not bool((out == SENTINEL_F).any()) and not bool((out_l == SENTINEL_L).any())


ARGUMENT_ERRORS = [
    ("crop_i past the edge", 5, dict(crop0=(3, 0))),
    ("crop_j past the edge", 5, dict(crop0=(0, 3))),
    ("oh > H", 6, dict(out_size=(10, 11))),
    ("ow > W", 6, dict(out_size=(7, 14))),
    ("an order with a repeat", 5, dict(order0=[0, 0, 1, 2])),
    ("an order entry of 4", 5, dict(order0=[0, 1, 2, 4])),
    ("a label with no out_label", 9, dict(out_label=False)),
]


@pytest.mark.parametrize("what,arg,kw", ARGUMENT_ERRORS, ids=[e[0].replace(" ", "_") for e in ARGUMENT_ERRORS])
def test_argument_errors_launch_nothing(ops, what, arg, kw):
    L = _lib()
    c = an.build_case("batch17")
    rc, _, _, intact = _abi(ops, c, **kw)
    assert rc == -1000 - arg, (what, rc)                  # UCSA_ERR_ARG - k
    with pytest.raises(L.UcsaError, match=f"code {-1000 - arg}"):
        L.check(rc, "ucsa_augment")
    assert intact(everything=True), f"{what}: something was written"
    # the same through the wrapper (it owns out_label, so that one cannot occur)
    if "out_label" not in kw:
        params = [dict(q) for q in c.params]
        if "crop0" in kw:
            params[0].update(crop_i=kw["crop0"][0], crop_j=kw["crop0"][1])
        if "order0" in kw:
            params[0]["order"] = kw["order0"]
        with pytest.raises(L.UcsaError):
            ops.augment(_dev(c.img), _dev(c.label, torch.int64), params, kw.get("out_size", c.out_size))


def test_empty_batch_returns_cleanly(ops):
    c = an.build_case("batch1")
    rc, _, _, intact = _abi(ops, c, B=0)
    assert rc == 0 and intact(everything=True)
    out, out_l = ops.augment(torch.empty(0, 3, 9, 13, device="cuda"),
                             torch.empty(0, 9, 13, dtype=torch.int64, device="cuda"), [], (7, 11))
    assert tuple(out.shape) == (0, 3, 7, 11) and tuple(out_l.shape) == (0, 7, 11)
    out, out_l = ops.augment(torch.empty(0, 3, 9, 13, device="cuda"), None, [])
    assert tuple(out.shape) == (0, 3, 9, 13) and out_l is None
    with pytest.raises(_lib().UcsaError):
        ops.augment(_dev(c.img), None, [])                # one params entry per image
