"""conv3x3_wrw_kernel + conv3x3_wrw_finish_kernel (row bands with a
rolling halo, one swapped-halves LDS image per operand, per-slab
partials summed in a fixed order) against an fp64 CPU weight gradient of
the bf16-rounded inputs.

Bound. A product of two bf16 numbers is exact in fp32, so the only error
is that of the fp32 summation of the M = B*H*W terms of one dW element.
Whatever the order (MFMA chains, waves, slabs), with A = sum |gy| |x|
over the same terms,
    |dw - ref| <= M * 2^-24 * A.
db is the same kind of sum of M unit-scale terms and keeps the tolerance
of test_conv3x3_stream.py::test_bias_gradient.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, K) of the kernel instances the flagship decoder runs, plus the
# 48-channel one (three c-groups in one wave, a half-empty k tile)
INSTANCES = [(16, 16), (16, 4), (32, 32), (32, 16), (32, 4), (64, 64),
             (64, 32), (64, 4), (48, 24)]


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, K):
    """Inputs, the fp64 reference and its abs-sum, computed once."""
    assert B * H * W <= 2048
    g = torch.Generator().manual_seed(1000 * C + 10 * K + W)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    gy = torch.randn(B, K, H, W, generator=g).to(torch.bfloat16)

    def wgrad(xx, gg):
        w = torch.zeros(K, C, 3, 3, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.pad(xx, (1, 1, 1, 1), mode="reflect"), w)
        return torch.autograd.grad(y, w, gg)[0]

    return dict(x=x, gy=gy, dw=wgrad(x.double(), gy.double()),
                dw_abs=wgrad(x.double().abs(), gy.double().abs()))


def _flat(t):
    return (t.to("cuda:0").contiguous(memory_format=torch.channels_last)
            .permute(0, 2, 3, 1).reshape(-1))


def _check(dw, B, C, H, W, K, what):
    c = _case(B, C, H, W, K)
    assert dw.dtype == torch.float32 and dw.shape == (K, C, 3, 3)
    err = (dw.double().cpu() - c["dw"]).abs()
    bound = B * H * W * 2.0 ** -24 * c["dw_abs"]
    worst = (err / bound).max().item()
    print(f"{what} {B, C, H, W, K}: max err/bound {worst:.3f}")
    assert worst <= 1.0


def _run(B, C, H, W, K, **kw):
    from mine_amd.ops.backend import get_extension
    ext = get_extension(required=True)
    c = _case(B, C, H, W, K)
    return ext.conv3x3_wrw(_flat(c["x"]), _flat(c["gy"]), B, H, W, C, K, **kw)


def _run_bias(B, C, H, W, K, **kw):
    from mine_amd.ops.backend import get_extension
    ext = get_extension(required=True)
    c = _case(B, C, H, W, K)
    return ext.conv3x3_wrw_bias(_flat(c["x"]), _flat(c["gy"]), B, H, W, C, K,
                                **kw)


# H = 9: odd row count, reflection at both ends, a one-row last band;
# W = 70: a partial 32-pixel chunk
@pytest.mark.parametrize("C,K", INSTANCES)
def test_per_instance(C, K):
    _check(_run(2, C, 9, 70, K), 2, C, 9, 70, K, "wrw")


# the 32-pixel chunk: one below, on, one past
@pytest.mark.parametrize("W", [31, 32, 33])
def test_chunk_boundary(W):
    _check(_run(2, 16, 9, W, 16), 2, 16, 9, W, 16, "chunk")


# the column tile is 384 / max(C/16, k tiles) pixels, so four widths
# ship: 384 (C = K = 16), 192 (C = 32: two c-groups x two pixel halves,
# partials added through LDS), 128 (C = 48: three c-groups per wave) and
# 96 (C = 64). One below, on, and one past each; one past adds a second
# tile one pixel wide.
@pytest.mark.parametrize("C,K,H,W", [
    (16, 16, 2, 383), (16, 16, 2, 384), (16, 16, 2, 385),
    (32, 32, 2, 191), (32, 32, 2, 192), (32, 32, 2, 193),
    (48, 24, 4, 127), (48, 24, 4, 128), (48, 24, 4, 129),
    (64, 64, 9, 95), (64, 64, 9, 96), (64, 64, 9, 97)])
def test_column_tile_boundary(C, K, H, W):
    _check(_run(2, C, H, W, K), 2, C, H, W, K, "tile")


# the 4-channel (8-byte) path across a column-tile boundary, on every
# tile width it ships with: channels 4..15 of the gy image must still be
# zero in the second tile
@pytest.mark.parametrize("C,H,W", [(16, 2, 385), (16, 2, 420), (32, 4, 193),
                                   (48, 4, 129), (64, 9, 97)])
def test_four_channel_second_tile(C, H, W):
    _check(_run(2, C, H, W, 4), 2, C, H, W, 4, "k4 tile")
    dw, db = _run_bias(2, C, H, W, 4)
    _check(dw, 2, C, H, W, 4, "k4 tile+bias")
    gy = _case(2, C, H, W, 4)["gy"].cuda()
    torch.testing.assert_close(db, gy.float().sum((0, 2, 3)), rtol=1e-5,
                               atol=1e-4 * (2 * H * W) ** 0.5)


# K neither 4 nor a multiple of 8: the binding zero-pads gy to the next
# multiple of 8 (K = 3, 12 -> one padded octet; K = 20 -> a second k
# tile that is half padding); dW and db keep K rows
@pytest.mark.parametrize("C,K", [(16, 3), (16, 12), (32, 20), (64, 1)])
def test_padded_k(C, K):
    B, H, W = 2, 9, 70
    dw, db = _run_bias(B, C, H, W, K)
    _check(dw, B, C, H, W, K, "padded K")
    _check(_run(B, C, H, W, K), B, C, H, W, K, "padded K, no bias")
    gy = _case(B, C, H, W, K)["gy"].cuda()
    assert db.shape == (K,)
    torch.testing.assert_close(db, gy.float().sum((0, 2, 3)), rtol=1e-5,
                               atol=1e-4 * (B * H * W) ** 0.5)


# the gate's minimum; fewer rows than a band plus its halo
@pytest.mark.parametrize("H,W", [(8, 48), (3, 300)])
def test_small_images(H, W):
    _check(_run(2, 16, H, W, 16), 2, 16, H, W, 16, "small")


# 2 x 9 rows: one slab; a boundary at the image boundary; boundaries
# inside both images
@pytest.mark.parametrize("slabs", [1, 2, 3])
@pytest.mark.parametrize("C,K", [(16, 16), (32, 4), (64, 64)])
def test_forced_slabs(C, K, slabs):
    _check(_run(2, C, 9, 70, K, max_slabs=slabs), 2, C, 9, 70, K,
           f"slabs={slabs}")


@pytest.mark.parametrize("slabs", [0, 7])
def test_more_slabs_than_rows(slabs):
    _check(_run(1, 16, 3, 70, 16, max_slabs=slabs), 1, 16, 3, 70, 16,
           f"slabs={slabs}")


@pytest.mark.parametrize("C,K", [(16, 16), (32, 4), (64, 64)])
def test_bitwise_reproducible(C, K):
    """The order-fixed reduction: equal inputs give equal bits."""
    a = _run(2, C, 9, 70, K)
    b = _run(2, C, 9, 70, K)
    assert torch.equal(a, b)
    dw1, db1 = _run_bias(2, C, 9, 70, K)
    dw2, db2 = _run_bias(2, C, 9, 70, K)
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)
    assert torch.equal(dw1, a)       # the bias pass leaves dW alone


@pytest.mark.parametrize("slabs", [0, 3])
@pytest.mark.parametrize("K", [16, 4])
def test_bias_gradient_same_pass(K, slabs):
    B, C, H, W = 2, 16, 9, 70
    dw, db = _run_bias(B, C, H, W, K, max_slabs=slabs)
    _check(dw, B, C, H, W, K, "wrw+bias")
    gy = _case(B, C, H, W, K)["gy"].cuda()
    ref = gy.float().sum((0, 2, 3))
    M = B * H * W
    assert db.dtype == torch.float32 and db.shape == (K,)
    print(f"db K={K}: max abs err {(db - ref).abs().max().item():.3e}")
    torch.testing.assert_close(db, ref, rtol=1e-5, atol=1e-4 * M ** 0.5)


def test_unsupported_channels_are_an_error():
    from mine_amd.ops.backend import get_extension
    ext = get_extension(required=True)
    x = torch.zeros(2 * 4 * 8 * 24, device="cuda:0", dtype=torch.bfloat16)
    gy = torch.zeros(2 * 4 * 8 * 8, device="cuda:0", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.conv3x3_wrw(x, gy, 2, 4, 8, 24, 8)
