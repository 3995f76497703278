"""CPU side of the fp16 element type: the weight packs take an output
dtype, default bf16."""
import pytest
import torch

from mine_amd.ops.conv import (_pack_lut, _pack_lut_bwd, pack_weights,
                               pack_weights_bwd)


def _gather(w, lut, dtype):
    flat = torch.cat((w.reshape(-1).to(dtype), torch.zeros(1, dtype=dtype)))
    return flat[lut]


@pytest.mark.parametrize("K,C", [(16, 16), (4, 16), (24, 48)])
def test_pack_weights_dtype(K, C):
    g = torch.Generator().manual_seed(K * 100 + C)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.2
    cpu = torch.device("cpu")
    for flip in (False, True):
        lut = _pack_lut(K, C, flip, cpu)
        p16 = pack_weights(w, flip, dtype=torch.float16)
        assert p16.dtype == torch.float16
        assert torch.equal(p16, _gather(w, lut, torch.float16))
        pdef = pack_weights(w, flip)
        assert pdef.dtype == torch.bfloat16
        assert torch.equal(pdef, _gather(w, lut, torch.bfloat16))
        assert torch.equal(pack_weights(w, flip, dtype=torch.bfloat16), pdef)
    # the 11-bit significand survives: some packed value is no bf16 number
    p16 = pack_weights(w, dtype=torch.float16)
    assert (p16.to(torch.bfloat16).to(torch.float16) != p16).any()


@pytest.mark.parametrize("K,C", [(16, 16), (4, 16), (24, 48)])
def test_pack_weights_bwd_dtype(K, C):
    g = torch.Generator().manual_seed(K * 100 + C + 1)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.2
    lut = _pack_lut_bwd(K, C, torch.device("cpu"))
    p16 = pack_weights_bwd(w, dtype=torch.float16)
    assert p16.dtype == torch.float16
    assert torch.equal(p16, _gather(w, lut, torch.float16))
    pdef = pack_weights_bwd(w)
    assert pdef.dtype == torch.bfloat16
    assert torch.equal(pdef, _gather(w, lut, torch.bfloat16))


def test_pack_rejects_other_dtypes():
    w = torch.zeros(16, 16, 3, 3)
    with pytest.raises(ValueError):
        pack_weights(w, dtype=torch.float32)
