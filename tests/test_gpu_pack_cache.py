"""The packed-weight cache of SemanticNeRFNetwork on the device: every pack form
of every net, the fp16 table and the rounded sigma packs are what a fresh call of
the ``ops`` function gives (bit for bit), are returned again while the parameters
stand, and are refreshed IN PLACE -- same ``data_ptr`` -- after an update.

The rounded sigma packs (``_pack_rounded_sigma``, train_precision="tcnn") are the
one exception to "in place": they are packed from a rounded copy of the parameters
into new buffers, as they always were (tests/golden/dispatch_trace.json holds that
call without ``out``), so for them the contents are checked and not the address.
One of the 21 form x net pairs does not exist in the library, the transposed f16
pack of the sigma net: for it the test holds the error and an untouched cache.
"""
import pytest
import torch

from ucsa_neural_rendering_amd import ops
from ucsa_neural_rendering_amd._lib import UcsaError
from ucsa_neural_rendering_amd.nerf.network_tcnn_semantics import (NETS, PACK_FORMS,
                                                                   SemanticNeRFNetwork)

pytestmark = pytest.mark.gpu
C = 5


@pytest.fixture(scope="module")
def net():
    return SemanticNeRFNetwork(num_semantic_classes=C, seed=0).to("cuda")


def _update(p):
    with torch.no_grad():
        p.mul_(1.25).add_(0.01)


@pytest.mark.parametrize("name", list(NETS))
@pytest.mark.parametrize("form", list(PACK_FORMS))
def test_pack_forms(net, form, name):
    assert sorted(PACK_FORMS) == sorted(("f32", "t", "h", "th", "x3", "t_x3", "h2"))
    mlp = getattr(net, NETS[name])
    fresh = lambda: getattr(ops, PACK_FORMS[form][0])(mlp.kind, mlp.params, C)  # noqa: E731
    if (form, name) == ("th", "sigma"):
        # the library has no transposed f16 pack of the sigma net (its backward is
        # fp32 or bf16x2): the refusal comes through the cache, which keeps nothing
        with pytest.raises(UcsaError, match="ucsa_mlp_pack_t_f16"):
            fresh()
        with pytest.raises(UcsaError, match="ucsa_mlp_pack_t_f16"):
            net._pack(form, name)
        assert "sigma_th" not in net._packed
        return
    first = net._pack(form, name)
    assert torch.equal(first, fresh())
    assert net._pack(form, name) is first
    assert net._packed[name + PACK_FORMS[form][1]][1] is first
    ptr = first.data_ptr()
    _update(mlp.params)
    again = net._pack(form, name)
    assert again.data_ptr() == ptr
    assert torch.equal(again, fresh())
    if form == "h2":      # the default guard ("weights") raised the net's range word
        torch.cuda.synchronize()
        bits = int(net._h2_flags[name][0]) & 0xFFFFFFFF
        assert 0 < bits < net.H2_BITS_LIMIT


def test_table_half(net):
    first = net._table_half()
    assert torch.equal(first, ops.table_to_half(net.encoder.params))
    assert net._table_half() is first and net._packed["table_h16"][1] is first
    ptr = first.data_ptr()
    _update(net.encoder.params)
    again = net._table_half()
    assert again.data_ptr() == ptr
    assert torch.equal(again, ops.table_to_half(net.encoder.params))


def test_rounded_sigma_packs(net):
    mlp = net.sigma_net

    def fresh():
        r = mlp.params.detach().half().float()
        return ops.mlp_pack(mlp.kind, r, C), ops.mlp_pack_t(mlp.kind, r, C)
    first = net._pack_rounded_sigma()
    assert all(torch.equal(a, b) for a, b in zip(first, fresh()))
    assert net._pack_rounded_sigma() is first and net._packed["sigma_r16"][1] is first
    assert net._pack("r16", "sigma") is first[0] and net._pack("r16_t", "sigma") is first[1]
    _update(mlp.params)
    again = net._pack_rounded_sigma()
    assert again is not first
    assert all(torch.equal(a, b) for a, b in zip(again, fresh()))
