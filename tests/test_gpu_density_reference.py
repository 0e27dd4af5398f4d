"""Every entry point of the density pass -- ``ucsa_sigma_mlp_fwd``, ``_f16``,
``_f16_h``, ``_x3``, ``_h2``, ``ucsa_sigma_mlp_fwd_scatter`` in its four modes,
``ucsa_density_sorted`` in modes 2 / 3 with 8, 12 or 16 levels encoded inside --
against the float64 reference of tests/density_numpy.py: every ``h`` element
within a bound derived from counting rounding steps, every ``sigma`` inside
its interval.  One test id = one entry point on one case.  Outputs (and the
fused path's feature workspace) are filled with NaN before every call.  No
flat tolerance, no exempt rows, no L2 fallback; the bit-identity tests of
tests/test_gpu_parity.py stay what they are.

tests/test_density_reference_cpu.py holds the reference against the oracle and
shows that the same ``compare_density`` call rejects wrong implementations.

Worst err / bound per entry point and case family, as printed at the end of a
run on an MI355X: docs/DESIGN_NOTEBOOK.md, section DN."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle.fixtures import hip_network_from_oracle, lively_oracle_field
from tests import density_numpy as dn
from tests import hashgrid_numpy as hn
from tests import shade_numpy as sn

pytestmark = pytest.mark.gpu

# entry point -> (reference mode, pack, features handed over as fp16)
PLAIN = {"sigma_mlp_fwd": ("fp32", "mlp_pack", False),
         "sigma_mlp_fwd_f16": ("f16", "mlp_pack_f16", False),
         "sigma_mlp_fwd_f16_h": ("f16", "mlp_pack_f16", True),
         "sigma_mlp_fwd_x3": ("x3", "mlp_pack_x3", False),
         "sigma_mlp_fwd_h2": ("h2", "mlp_pack_h2", False)}
SCATTER = {0: PLAIN["sigma_mlp_fwd"], 1: PLAIN["sigma_mlp_fwd_f16_h"],
           2: PLAIN["sigma_mlp_fwd_x3"], 3: PLAIN["sigma_mlp_fwd_h2"]}
FUSED = [(mode, n_enc) for mode in (2, 3) for n_enc in (8, 12, 16)]
SIZE_CASES = [(M, "w0") for M in dn.SIZES] + [(M, "w8") for M in (17, 129, 1025)]


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    seen = set(sn.WORST)
    yield _ops
    new = sorted(k for k in sn.WORST if k not in seen)
    if new:
        print("\nworst err / bound of h per entry point and case family:")
        for k in new:
            print(f"  {k}: {sn.WORST[k]:.3f}")


@functools.lru_cache(maxsize=None)
def field():
    return lively_oracle_field()


@functools.lru_cache(maxsize=None)
def weights(name):
    return field().sigma_params.numpy() if name == "w0" else dn.scaled_weights()


@functools.lru_cache(maxsize=None)
def rows_case(family, key, wname):
    if family == "sizes":
        return dn.case_sizes(key)
    if family == "magnitudes":
        return dn.case_magnitudes(f16=bool(key))
    return dn.case_exp(weights(wname))


@functools.lru_cache(maxsize=None)
def rows_ref(family, key, wname, mode):
    return dn.density_rows(rows_case(family, key, wname).x, weights(wname), mode)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def _packed(pack, wname):
    from ucsa_neural_rendering_amd import _lib
    from ucsa_neural_rendering_amd import ops as _ops
    return getattr(_ops, pack)(_lib.MLP_SIGMA, _dev(weights(wname)))


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_plain(ops, entry, feat, wname):
    """feat [16, M, 2] fp32 on the device -> (h [M, 16], sigma [M]) through the
    C entry point, outputs prefilled with NaN."""
    from ucsa_neural_rendering_amd import _lib
    _, pack, half = PLAIN[entry]
    M = feat.shape[1]
    if half:
        feat = feat.half()
    h, sigma = _nan(M, 16), _nan(M)
    p = ops._ptr
    _lib.check(getattr(_lib.lib(), "ucsa_" + entry)(p(feat), p(_packed(pack, wname)), M, 16, p(h),
                                                    p(sigma), ops._stream()), "ucsa_" + entry)
    torch.cuda.synchronize()
    return h, sigma


def run_scatter(ops, mode, feat, wname, slot, rows):
    """-> (h [rows, 16], sigma [rows]) prefilled with NaN, row slot[m] written"""
    from ucsa_neural_rendering_amd import _lib
    _, pack, half = SCATTER[mode]
    M = feat.shape[1]
    if half:
        feat = feat.half()
    h, sigma = _nan(rows, 16), _nan(rows)
    p = ops._ptr
    _lib.check(_lib.lib().ucsa_sigma_mlp_fwd_scatter(mode, p(feat), p(_packed(pack, wname)), M, 16,
                                                     p(slot), p(h), p(sigma), ops._stream()),
               "ucsa_sigma_mlp_fwd_scatter")
    torch.cuda.synchronize()
    return h, sigma


# ---------------------------------------------------------------------------
# the plain forwards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", SIZE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("entry", list(PLAIN))
def test_sizes(ops, entry, case):
    """16-column blocks, the wave's span (64 / 128 samples), the workgroup's
    (256 / 512), clamped loads of row M - 1; the all-zero row is exact."""
    M, wname = case
    c = rows_case("sizes", M, wname)
    h, sigma = run_plain(ops, entry, _dev(dn.to_feat(c.x)), wname)
    dn.compare_density(h, sigma, rows_ref("sizes", M, wname, PLAIN[entry][0]), f"{entry} sizes @ {c.name}")


@pytest.mark.parametrize("wname", ["w0", "w8"])
@pytest.mark.parametrize("entry", list(PLAIN))
def test_magnitudes(ops, entry, wname):
    """features from 2^-30 to 2^10 (f16x2's absolute floor, fp16 subnormals and
    zeros), the grid's initial scale, an exact zero row; the fp16 entry points
    besides +-65504 and 65520, which is inf in fp16."""
    f16 = PLAIN[entry][0] == "f16"
    c = rows_case("magnitudes", int(f16), wname)
    h, sigma = run_plain(ops, entry, _dev(dn.to_feat(c.x)), wname)
    ref = rows_ref("magnitudes", int(f16), wname, PLAIN[entry][0])
    dn.compare_density(h, sigma, ref, f"{entry} magnitudes @ {c.name}")
    assert bool((h[c.zero_row] == 0).all()) and float(sigma[c.zero_row]) == 1.0


@pytest.mark.parametrize("wname", ["w0", "w8"])
@pytest.mark.parametrize("entry", ["sigma_mlp_fwd", "sigma_mlp_fwd_x3", "sigma_mlp_fwd_h2"])
def test_exp(ops, entry, wname):
    """h0 from -110 to 200: zero and subnormal sigma, the overflow straddle, inf"""
    c = rows_case("exp", None, wname)
    ref = rows_ref("exp", None, wname, PLAIN[entry][0])
    h, sigma = run_plain(ops, entry, _dev(dn.to_feat(c.x)), wname)
    print("h0:", h[:, 0].tolist(), "sigma:", sigma.tolist())
    dn.compare_density(h, sigma, ref, f"{entry} exp @ {c.name}")
    s, t = sigma.cpu().numpy(), list(c.targets)
    assert np.isposinf(s[t.index(200.0)]) and s[t.index(0.0)] == 1.0 and np.isfinite(s[t.index(20.0)])


@pytest.mark.parametrize("entry", list(PLAIN))
def test_wrap(ops, entry):
    """M = the entry point's grid-stride threshold + 17: rows below P = 4096
    against float64, every other row bit-equal to row m mod P."""
    mode = PLAIN[entry][0]
    M, P = dn.WRAP_M[mode], dn.WRAP_P
    c = rows_case("sizes", P, "w0")
    idx = torch.arange(M, device="cuda") % P
    feat = _dev(dn.to_feat(c.x))[:, idx, :].contiguous()
    h, sigma = run_plain(ops, entry, feat, "w0")
    del feat
    dn.compare_density(h[:P], sigma[:P], rows_ref("sizes", P, "w0", mode), f"{entry} wrap @ M={M}")
    assert torch.equal(_bits(h), _bits(h[:P])[idx]), "a row past the wrap differs from its copy"
    assert torch.equal(_bits(sigma), _bits(sigma[:P])[idx])


@pytest.mark.parametrize("M", [17, 257])
def test_f16_entry_points_agree(ops, M):
    """``_f16`` (rounds fp32 features on load) and ``_f16_h`` (reads them
    rounded): the same bits, as include/ucsa_hip.h promises"""
    for x in (rows_case("sizes", M, "w0").x, rows_case("magnitudes", 0, "w0").x):
        feat = _dev(dn.to_feat(x))
        h0, s0 = run_plain(ops, "sigma_mlp_fwd_f16", feat, "w0")
        h1, s1 = run_plain(ops, "sigma_mlp_fwd_f16_h", feat, "w0")
        assert torch.equal(_bits(h0), _bits(h1)) and torch.equal(_bits(s0), _bits(s1))


POISON = [(48, 21), (17, 16), (65, 64)]       # (M, poisoned row): column 5 of block 1; row M - 1


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", POISON, ids=lambda w: f"M{w[0]}row{w[1]}")
@pytest.mark.parametrize("entry", list(PLAIN))
def test_poison(ops, entry, where, value):
    """one non-finite feature: every OTHER row keeps the bits of the clean run
    (MFMA columns do not mix; row M - 1's clamped copies write nothing)"""
    M, row = where
    x = dn.case_sizes(M).x.copy()
    clean_h, clean_s = run_plain(ops, entry, _dev(dn.to_feat(x)), "w0")
    x[row, 2 * 5 + 1] = value
    h, s = run_plain(ops, entry, _dev(dn.to_feat(x)), "w0")
    keep = torch.arange(M, device="cuda") != row
    assert torch.equal(_bits(h)[keep], _bits(clean_h)[keep])
    assert torch.equal(_bits(s)[keep], _bits(clean_s)[keep])
    # (the poisoned row itself is not held to anything: a NaN pre-activation
    # passes the kernels' ReLU as 0, mfma_mlp_h2.h "RANGE")


# ---------------------------------------------------------------------------
# scatter
# ---------------------------------------------------------------------------
SCATTER_M = 300


@pytest.mark.parametrize("kind", ["random", "identity", "reverse"])
@pytest.mark.parametrize("mode", list(SCATTER))
def test_scatter(ops, mode, kind):
    """row slot[m] of the outputs holds sample m"""
    c = rows_case("sizes", SCATTER_M, "w0")
    slot = dn.slots(SCATTER_M, kind)
    h, sigma = run_scatter(ops, mode, _dev(dn.to_feat(c.x)), "w0", _dev(slot, torch.int32), SCATTER_M)
    sl = torch.from_numpy(slot).long().cuda()
    dn.compare_density(h[sl], sigma[sl], rows_ref("sizes", SCATTER_M, "w0", SCATTER[mode][0]),
                       f"sigma_mlp_fwd_scatter[{mode}] scatter @ {kind}")


@pytest.mark.parametrize("mode", list(SCATTER))
def test_scatter_into_even_rows(ops, mode):
    """buffers of 2 M rows, slot = 2 x a permutation: every even row is written
    (M writes into M rows: each once), every odd row keeps its NaN bytes"""
    c = rows_case("sizes", SCATTER_M, "w0")
    slot = 2 * dn.slots(SCATTER_M, "random", seed=1)
    h, sigma = run_scatter(ops, mode, _dev(dn.to_feat(c.x)), "w0", _dev(slot, torch.int32), 2 * SCATTER_M)
    sl = torch.from_numpy(slot).long().cuda()
    dn.compare_density(h[sl], sigma[sl], rows_ref("sizes", SCATTER_M, "w0", SCATTER[mode][0]),
                       f"sigma_mlp_fwd_scatter[{mode}] scatter @ even rows")
    fill_h, fill_s = _nan(SCATTER_M, 16), _nan(SCATTER_M)
    assert torch.equal(_bits(h[1::2]), _bits(fill_h)) and torch.equal(_bits(sigma[1::2]), _bits(fill_s))
    assert bool(torch.isfinite(h[0::2]).all())


# ---------------------------------------------------------------------------
# encoder + net in one call
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net():
    return hip_network_from_oracle(field()).eval()


@functools.lru_cache(maxsize=None)
def fused_case(H, W, T):
    n = net()
    f = n._field()
    c = dn.case_fused(H, W, T, field().bound)
    c.levels = hn.levels_of(f["grid"])
    assert c.levels == hn.levels_of(field().grid), "the library's level table is not the oracle's"
    c.table = field().grid_params.numpy().reshape(-1, 2)
    c.aabb = n._aabb_list(False)
    assert [float(v) for v in c.aabb] == hn.aabb_of(field().bound)
    return c


@functools.lru_cache(maxsize=None)
def fused_ref(H, W, T, mode):
    c = fused_case(H, W, T)
    return dn.density_rays(c.levels, field().bound, c.table, c.o, c.d, c.z, c.aabb, weights("w0"), mode)


@contextlib.contextmanager
def density_levels(ops, monkeypatch, n_enc):
    try:
        with monkeypatch.context() as m:
            m.setenv("UCSA_DENSITY_LEVELS", str(n_enc))
            ops.env_reload()
            yield
    finally:
        ops.env_reload()


FUSED_SHAPES = [("depth",) + s for s in dn.FUSED_DEPTH] + [("index",) + s for s in dn.FUSED_INDEX]


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}x{s[3]}")
@pytest.mark.parametrize("config", FUSED, ids=lambda c: f"mode{c[0]}-enc{c[1]}")
def test_fused(ops, monkeypatch, config, shape):
    """``ucsa_density_sorted`` against ``density_rays``: one wave only, one and
    two sample blocks per tile, a one-pixel tile, ragged tiles, fixed-width
    slabs, 64 sample blocks per tile; levels from the LDS tile and from the
    workspace at each split.  The workspace starts as NaN: a level read from
    it that the per-level encoder did not write shows."""
    from ucsa_neural_rendering_amd import _lib
    (mode, n_enc), (order, H, W, T) = config, shape
    name, pack, _ = SCATTER[mode]
    c, ref = fused_case(H, W, T), fused_ref(H, W, T, name)
    f = net()._field()
    o, d, z = _dev(c.o), _dev(c.d), _dev(c.z)
    N, M = H * W, H * W * T
    zs, pix, slot = (ops.tile_depth_order if order == "depth" else ops.tile_index_order)(z, W)
    assert torch.equal(torch.sort(slot.long()).values, torch.arange(M, device="cuda"))
    feat_ws, h, sigma = _nan(16, M, 2), _nan(M, 16), _nan(M)
    p = ops._ptr
    with density_levels(ops, monkeypatch, n_enc):
        _lib.check(_lib.lib().ucsa_density_sorted(
            mode, ctypes.byref(f["grid"]), p(f["table"]), p(o), p(d), p(zs), p(pix), p(slot),
            _lib.fvec(c.aabb), N, T, W, p(_packed(pack, "w0")), p(feat_ws), p(h), p(sigma),
            ops._stream()), "ucsa_density_sorted")
        torch.cuda.synchronize()
    dn.compare_density(h, sigma, ref, f"density_sorted[{name},{n_enc}] fused @ {order} {c.name}")
