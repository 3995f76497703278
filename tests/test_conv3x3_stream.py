"""conv3x3_fwd_kernel (compile-time C/K, swapped operands, padded LDS
image) against an fp64 CPU convolution of the bf16-rounded inputs.

Bounds. With A = conv(|x|, |w|) + |b| per output element, the kernel
does fp32 accumulation over <= 576 terms (error <= 2^-13 * A, generous
for 576 * 2^-24) and ONE bf16 rounding of the result (2^-9 relative,
bounded here by 2^-8 * |ref|):
    forward        |y  - ref| <= 2^-8 * |ref| + 2^-13 * A
The data gradient has a bf16 intermediate (the zero-embed conv output)
and the reflect fold then adds up to 4 such partials in fp32 before the
final rounding, so its rounding term is taken against the abs-sum A':
    data gradient  |gx - ref| <= 2^-8 * A'   + 2^-13 * A'
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (C, K) pairs of the kernel instances the flagship decoder runs, plus
# the 48-channel one (C/8 = 6, K-dim tail of two zero segments)
INSTANCES = [(16, 16), (16, 4), (32, 32), (32, 16), (32, 4), (64, 64),
             (64, 32), (64, 4), (48, 24)]


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, K):
    """Inputs and fp64 references for one shape, computed once."""
    g = torch.Generator().manual_seed(1000 * C + 10 * K + W)
    x = torch.randn(B, C, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(K, C, 3, 3, generator=g) * 0.2)
    b = torch.randn(K, generator=g) * 0.1
    gy = torch.randn(B, K, H, W, generator=g).to(torch.bfloat16)
    wq = w.to(torch.bfloat16).double()

    def conv(xx, ww, bb):
        return F.conv2d(F.pad(xx, (1, 1, 1, 1), mode="reflect"), ww, bb)

    xd = x.double().requires_grad_(True)
    y = conv(xd, wq, b.double())
    (gx,) = torch.autograd.grad(y, xd, gy.double())
    xa = x.double().abs().requires_grad_(True)
    ya = conv(xa, wq.abs(), b.double().abs())
    (gxa,) = torch.autograd.grad(ya, xa, gy.double().abs())
    return dict(x=x, w=w, b=b, gy=gy, y=y.detach(), y_abs=ya.detach(),
                gx=gx, gx_abs=gxa)


def _cl(t):
    return t.to("cuda:0").contiguous(memory_format=torch.channels_last)


def _check_fwd(B, C, H, W, K):
    from mine_amd.ops.conv import conv3x3_reflect
    c = _case(B, C, H, W, K)
    with torch.no_grad():
        y = conv3x3_reflect(_cl(c["x"]), c["w"].cuda(), c["b"].cuda())
    assert y.dtype == torch.bfloat16 and y.shape == (B, K, H, W)
    err = (y.double().cpu() - c["y"]).abs()
    bound = 2.0 ** -8 * c["y"].abs() + 2.0 ** -13 * c["y_abs"]
    worst = (err / bound).max().item()
    print(f"fwd {B, C, H, W, K}: max err/bound {worst:.3f}")
    assert worst <= 1.0


def _check_bwd_data(B, C, H, W, K):
    from mine_amd.ops.conv import conv3x3_bwd_data
    c = _case(B, C, H, W, K)
    gx = conv3x3_bwd_data(_cl(c["gy"]), c["w"].cuda())
    assert gx.dtype == torch.bfloat16 and gx.shape == (B, C, H, W)
    err = (gx.double().cpu() - c["gx"]).abs()
    bound = (2.0 ** -8 + 2.0 ** -13) * c["gx_abs"]
    worst = (err / bound).max().item()
    print(f"bwd_data {B, C, H, W, K}: max err/bound {worst:.3f}")
    assert worst <= 1.0


# H = 9: odd row count, reflection at both ends, a partial row tile;
# W = 70: a second column tile with a partial 16-pixel group
@pytest.mark.parametrize("C,K", INSTANCES)
def test_forward_per_instance(C, K):
    _check_fwd(2, C, 9, 70, K)


@pytest.mark.parametrize("C,K", INSTANCES)
def test_bwd_data_per_instance(C, K):
    _check_bwd_data(2, C, 9, 70, K)


# the gate's minimum; exactly one tile; three tiles, the last 2 wide
@pytest.mark.parametrize("H,W", [(8, 48), (9, 64), (9, 130)])
def test_forward_edges(H, W):
    _check_fwd(2, 16, H, W, 16)


# logical width W+2 = 64 / 65 / 66: ends on, one past, two past a tile
@pytest.mark.parametrize("W", [62, 63, 64])
@pytest.mark.parametrize("K", [16, 4])
def test_bwd_data_tile_boundary(W, K):
    _check_bwd_data(2, 16, 10, W, K)


def test_bwd_data_4ch_makes_no_padded_copy():
    """The 4-channel gradient goes to the kernel as it is: peak memory
    during the call is the packed weight + the (H+2,W+2) kernel output +
    the folded result, with no 8-channel copy of gy (which would be
    B*8*H*W*2 = 19840 bytes here). Slack: the caching allocator rounds
    each block up to 512 bytes; 8 blocks' worth covers the three
    tensors, the empty bias and the LUT lookup."""
    from mine_amd.ops.conv import conv3x3_bwd_data
    B, C, H, W, K = 2, 16, 10, 62, 4
    c = _case(B, C, H, W, K)
    gy, w = _cl(c["gy"]), c["w"].cuda()
    conv3x3_bwd_data(gy, w)          # builds and caches the LUT
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    gx = conv3x3_bwd_data(gy, w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    n_chunks = (9 * 1 + 3) // 4      # the K-dim of 8 (padded) channels
    need = (n_chunks * 64 * 8 * 2                   # packed weights
            + B * (H + 2) * (W + 2) * C * 2         # zero-embed output
            + B * H * W * C * 2)                    # folded gradient
    slack = 8 * 512
    print(f"peak {peak} B, needed {need} B, slack {slack} B")
    assert gx.shape == (B, C, H, W)
    assert peak <= need + slack
    assert B * 8 * H * W * 2 > slack  # a padded copy could not hide in it


@pytest.mark.parametrize("K", [16, 4])
def test_bias_gradient(K):
    """Bias gradient through autograd against gy.float().sum((0,2,3)):
    fp32 sums of M unit-scale terms."""
    from mine_amd.ops.conv import conv3x3_reflect
    B, C, H, W = 2, 16, 9, 70
    c = _case(B, C, H, W, K)
    x = _cl(c["x"]).requires_grad_(True)
    w = c["w"].cuda().requires_grad_(True)
    b = c["b"].cuda().requires_grad_(True)
    gy = _cl(c["gy"])
    conv3x3_reflect(x, w, b).backward(gy)
    ref = gy.float().sum((0, 2, 3))
    M = B * H * W
    torch.testing.assert_close(b.grad, ref, rtol=1e-5,
                               atol=1e-4 * M ** 0.5)
