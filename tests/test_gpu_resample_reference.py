"""``ops.resample`` (``ucsa_resample``, csrc/sampling.hip) against the float64
reference of tests/resample_numpy.py, sample by sample: every output must lie
in one of the intervals the reference allows for it (one per bin index and
guard branch that fp32 round-off may legitimately take), with bounds derived
there from counting rounding steps.  No sample is exempt and there is no
statistical fallback.  tests/test_resample_reference_cpu.py holds the
reference against the oracle and shows that the same check rejects wrong
kernels (which case rejects which mistake: ``KILLED_BY`` there).

The shapes cover every chunk situation of the two scans (T = 64 k + 1 and
64 k + 2, T = 3), the three register sorts with and without padding, the
in-LDS sort (t > 256) and dynamic LDS up to, at and past 64 KiB.

Worst |kernel - v| / e per case, as printed at the end of a run on an MI355X:
docs/DESIGN_NOTEBOOK.md, "Float64 per-sample parity of hierarchical
resampling"."""
import functools

import numpy as np
import pytest
import torch

from tests import resample_numpy as rn

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def ops():
    from ucsa_neural_rendering_amd import ops as _ops
    yield _ops
    if rn.WORST:
        print("\nworst |kernel - v| / e per case:")
        for k in rn.WORST:
            print(f"  {k}: {rn.WORST[k]:.3f}")


@functools.lru_cache(maxsize=None)
def _case(name):
    c = rn.build_case(name)
    return c, rn.reference(c.z, c.sigma, c.u, c.density_scale)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", rn.CASE_NAMES)
def test_resample_matches_reference(ops, name):
    c, ref = _case(name)
    z, sigma, u = _dev(c.z), _dev(c.sigma), _dev(c.u)
    out = ops.resample(z, sigma, u, c.density_scale)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (c.N, c.t) and got.dtype == F32
    assert np.isfinite(got).all()
    # every sample in one of its allowed intervals
    rn.check(got, ref, name)
    # ascending per ray, exactly
    assert (np.diff(got, axis=1) >= 0).all()
    # inside the fp32 bin midpoints, exactly (evaluated here as the oracle does, not read back)
    zt = torch.from_numpy(c.z)
    bins = (zt[:, :-1] + 0.5 * (zt[:, 1:] - zt[:, :-1])).numpy()
    assert (got >= bins[:, :1]).all() and (got <= bins[:, -1:]).all()
    # a ray computed alone is the same ray inside the batch, bit for bit (the four waves
    # of a workgroup keep to their own LDS slices)
    for r in range(c.N) if c.N <= 9 else (0, 1, 2, 3, 4, 31, 62, 63):
        alone = ops.resample(z[r:r + 1], sigma[r:r + 1], u[r:r + 1], c.density_scale)
        assert torch.equal(alone[0], out[r]), f"ray {r} alone differs from ray {r} in the batch"


def test_lds_request_of_the_large_shapes():
    """what the size cases are there for: exactly 64 KiB, and more"""
    lds = lambda T, t: 16 * (3 * T + (1 << max(1, (t - 1).bit_length())))
    assert lds(1024, 1024) == 65536
    assert lds(1024, 1025) == 81920 and lds(2048, 1024) == 114688
    assert lds(4096, 4096) == 262144 > 163840 >= lds(2048, 4096)
    shapes = {(c[1], c[2]) for c in rn.CASES}
    assert {(1024, 1024), (1024, 1025), (2048, 1024)} <= shapes


@pytest.mark.parametrize("T,t,code", [(4096, 4096, -1004), (3414, 1, -1004), (2049, 2049, -1005),
                                      (2048, 4097, -1005), (2, 4, -1004)])
def test_unlaunchable_sizes_are_argument_errors(ops, T, t, code):
    """more LDS than a workgroup has (16 (3 T + tpad) bytes > 163,840), or a size
    outside the ABI: UcsaError with the argument's code, from the check -- a failed
    launch would carry a negative hipError_t instead -- and nothing is written"""
    from ucsa_neural_rendering_amd._lib import UcsaError
    z = torch.sort(torch.rand(2, T, device="cuda") * 7 + 0.2, -1)[0]
    sigma = torch.rand(2, T, device="cuda")
    u = torch.rand(2, t, device="cuda")
    with pytest.raises(UcsaError, match=rf"\(code {code}\)"):
        ops.resample(z, sigma, u, 1.0)
    torch.cuda.synchronize()
    # the library and the device are as they were
    c, ref = _case("T65_t40")
    got = ops.resample(_dev(c.z), _dev(c.sigma), _dev(c.u), c.density_scale).cpu().numpy()
    assert (rn.ratios(got, ref) <= 1.0).all()


def test_largest_launchable_size(ops):
    """T = 2048, t = 4096 asks for all 163,840 bytes"""
    rng = np.random.default_rng(77)
    z, sigma = rn._field("spike", rng, 3, 2048, 1.0)
    u = rn._uniforms("random", rng, 3, 2048, 4096)
    ref = rn.reference(z, sigma, u, 1.0)
    got = ops.resample(_dev(z), _dev(sigma), _dev(u), 1.0).cpu().numpy()
    rn.check(got, ref, "T2048_t4096")
    assert (np.diff(got, axis=1) >= 0).all()
