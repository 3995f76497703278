"""The fused 3x3 conv kernels (forward, data gradient, weight and bias
gradient) instantiated for fp16, against fp64 CPU references of the
fp16-rounded inputs.

Bounds (derived as in test_conv3x3_stream.py / test_conv3x3_wrw_stream.py,
with the fp16 half-ulp 2^-11 in place of bf16's 2^-9, each given the same
factor 2). With A = conv(|x|, |w|) + |b| per output element:
    forward        |y  - ref| <= 2^-10 * |ref| + 2^-13 * A + 2^-24
(one fp16 rounding; fp32 accumulation over <= 576 terms; 2^-24 is the
spacing of fp16 subnormals, whose rounding is absolute, not relative)
    data gradient  |gx - ref| <= (2^-10 + 2^-13) * A'
(an fp16 intermediate, up to 4 of which the reflect fold adds in fp32)
    weight grad    |dw - ref| <= M * 2^-24 * A''
(a product of two fp16 numbers has 22 significand bits and is exact in
fp32, so only the fp32 summation of the M = B*H*W terms errs).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16 = torch.float16


@functools.lru_cache(maxsize=None)
def _case(B, C, H, W, K):
    """fp16-rounded inputs and their fp64 references, computed once."""
    g = torch.Generator().manual_seed(1000 * C + 10 * K + W)
    x = torch.randn(B, C, H, W, generator=g).to(F16)
    w = torch.randn(K, C, 3, 3, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1
    gy = torch.randn(B, K, H, W, generator=g).to(F16)
    wq = w.to(F16).double()

    def conv(xx, ww, bb):
        return F.conv2d(F.pad(xx, (1, 1, 1, 1), mode="reflect"), ww, bb)

    def run(xx, ww, bb, gg):
        xx = xx.requires_grad_(True)
        ww = ww.requires_grad_(True)
        y = conv(xx, ww, bb)
        gx, gw = torch.autograd.grad(y, (xx, ww), gg)
        return y.detach(), gx, gw

    y, gx, _ = run(x.double(), wq.clone(), b.double(), gy.double())
    ya, gxa, _ = run(x.double().abs(), wq.abs(), b.double().abs(),
                     gy.double().abs())
    # the weight gradient does not depend on w
    _, _, dw = run(x.double(), torch.zeros_like(wq), None, gy.double())
    _, _, dwa = run(x.double().abs(), torch.zeros_like(wq), None,
                    gy.double().abs())
    return dict(x=x, w=w, b=b, gy=gy, y=y, y_abs=ya, gx=gx, gx_abs=gxa,
                dw=dw, dw_abs=dwa)


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _flat(t):
    return _cl(t).permute(0, 2, 3, 1).reshape(-1)


def _within(err, bound, what):
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err > 0, torch.full_like(err, 2.0),
                                    torch.zeros_like(err)))
    worst = ratio.max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert worst <= 1.0


def _check_fwd(B, C, H, W, K):
    from mine_amd.ops.conv import conv3x3_reflect
    c = _case(B, C, H, W, K)
    with torch.no_grad():
        y = conv3x3_reflect(_cl(c["x"]), c["w"].to(DEV), c["b"].to(DEV))
    assert y.dtype == F16 and y.shape == (B, K, H, W)
    err = (y.double().cpu() - c["y"]).abs()
    bound = 2.0 ** -10 * c["y"].abs() + 2.0 ** -13 * c["y_abs"] + 2.0 ** -24
    _within(err, bound, f"fwd {B, C, H, W, K}")


def _check_bwd_data(B, C, H, W, K):
    from mine_amd.ops.conv import conv3x3_bwd_data
    c = _case(B, C, H, W, K)
    gx = conv3x3_bwd_data(_cl(c["gy"]), c["w"].to(DEV))
    assert gx.dtype == F16 and gx.shape == (B, C, H, W)
    err = (gx.double().cpu() - c["gx"]).abs()
    bound = (2.0 ** -10 + 2.0 ** -13) * c["gx_abs"]
    _within(err, bound, f"bwd_data {B, C, H, W, K}")


INSTANCES = [(16, 16), (16, 4), (32, 4), (64, 64), (48, 24)]


@pytest.mark.parametrize("C,K", INSTANCES)
def test_forward(C, K):
    _check_fwd(2, C, 9, 70, K)


@pytest.mark.parametrize("C,K", INSTANCES)
def test_bwd_data(C, K):
    _check_bwd_data(2, C, 9, 70, K)


@pytest.mark.parametrize("H,W", [(8, 48), (9, 130)])
def test_forward_edges(H, W):
    _check_fwd(2, 16, H, W, 16)


@pytest.mark.parametrize("W", [62, 63, 64])
@pytest.mark.parametrize("K", [16, 4])
def test_bwd_data_tile_boundary(W, K):
    _check_bwd_data(2, 16, 10, W, K)


# ---------------------------------------------------------------------------
# fp16 inputs reach the MFMA as fp16: values 1 + k * 2^-10 need all 11
# significand bits, and 7 of 8 of them change under .to(bfloat16)
# ---------------------------------------------------------------------------

def _fine_values(shape, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 1024, shape, generator=g)
    x = (1.0 + k.double() * 2.0 ** -10).to(F16)
    assert (x.to(torch.bfloat16).to(F16) != x).float().mean() > 0.8
    return x


def _identity3x3(C):
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return w


def test_identity_conv3x3_is_exact():
    from mine_amd.ops.conv import conv3x3_reflect
    x = _cl(_fine_values((2, 16, 9, 70), 1))
    with torch.no_grad():
        y = conv3x3_reflect(x, _identity3x3(16).to(DEV), None)
    assert y.dtype == F16
    assert torch.equal(y, x)


def test_identity_conv1x1_igemm_is_exact():
    from mine_amd.ops.conv_general import conv2d_mfma
    x = _cl(_fine_values((2, 16, 9, 70), 2))
    w = torch.eye(16).view(16, 16, 1, 1).contiguous().to(DEV)
    with torch.no_grad():
        y = conv2d_mfma(x, w, None)
    assert y.dtype == F16
    assert torch.equal(y, x)


def test_identity_bwd_data_is_exact():
    """The fold adds only the zero ring to the edge pixels here."""
    from mine_amd.ops.conv import conv3x3_bwd_data
    gy = _cl(_fine_values((2, 16, 9, 70), 3))
    gx = conv3x3_bwd_data(gy, _identity3x3(16).to(DEV))
    assert gx.dtype == F16
    assert torch.equal(gx[:, :, 1:-1, 1:-1], gy[:, :, 1:-1, 1:-1])


def test_forward_makes_no_copy_of_the_activation():
    """Peak memory of a forward is the packed weights plus the output;
    slack as in test_bwd_data_4ch_makes_no_padded_copy (8 allocator
    blocks of 512 bytes). One 16-bit copy of x would not fit in it."""
    from mine_amd.ops.conv import conv3x3_reflect
    B, C, H, W, K = 2, 16, 10, 62, 16
    c = _case(B, C, H, W, K)
    x, w = _cl(c["x"]), c["w"].to(DEV)
    with torch.no_grad():
        conv3x3_reflect(x, w, None)      # builds and caches the LUT
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        y = conv3x3_reflect(x, w, None)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    n_chunks = (9 * (C // 8) + 3) // 4
    need = ((K + 15) // 16 * n_chunks * 64 * 8 * 2   # packed weights
            + B * H * W * K * 2)                     # output
    slack = 8 * 512
    print(f"peak {peak} B, needed {need} B, slack {slack} B")
    assert y.dtype == F16
    assert peak <= need + slack
    assert B * C * H * W * 2 > slack


# ---------------------------------------------------------------------------
# weight and bias gradient
# ---------------------------------------------------------------------------

def _check_wrw(B, C, H, W, K):
    from mine_amd.ops.backend import get_extension
    ext = get_extension(required=True)
    c = _case(B, C, H, W, K)
    xf, gf = _flat(c["x"]), _flat(c["gy"])
    dw = ext.conv3x3_wrw(xf, gf, B, H, W, C, K)
    dw2, db = ext.conv3x3_wrw_bias(xf, gf, B, H, W, C, K)
    M = B * H * W
    bound = M * 2.0 ** -24 * c["dw_abs"]
    for name, t in (("wrw", dw), ("wrw+bias", dw2)):
        assert t.dtype == torch.float32 and t.shape == (K, C, 3, 3)
        _within((t.double().cpu() - c["dw"]).abs(), bound,
                f"{name} {B, C, H, W, K}")
    assert db.dtype == torch.float32 and db.shape == (K,)
    ref = c["gy"].double().sum((0, 2, 3)).float()
    print(f"db: max abs err {(db.cpu() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(db.cpu(), ref, rtol=1e-5, atol=1e-4 * M ** 0.5)


@pytest.mark.parametrize("C,K", [(16, 16), (16, 4), (64, 64), (48, 24),
                                 (16, 12)])
def test_weight_and_bias_gradient(C, K):
    _check_wrw(2, C, 9, 70, K)


@pytest.mark.parametrize("C,K,H,W", [(16, 16, 2, 385), (64, 64, 9, 97)])
def test_weight_gradient_column_tiles(C, K, H, W):
    _check_wrw(2, C, H, W, K)


# ---------------------------------------------------------------------------
# fp16 range and dtype checks
# ---------------------------------------------------------------------------

def test_overflow_gives_inf():
    """The GradScaler has to see the overflow: no saturation."""
    from mine_amd.ops.conv import conv3x3_reflect
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 16, 9, 70, generator=g).to(F16)
    x[0, 3, 4, 30] = 60000.0
    with torch.no_grad():
        y = conv3x3_reflect(_cl(x), (2.0 * _identity3x3(16)).to(DEV), None)
    y = y.cpu()
    assert y[0, 3, 4, 30].item() == float("inf")
    inf = torch.isinf(y)
    assert inf.sum().item() == 1 and not torch.isnan(y).any()
    assert torch.equal(y[~inf], (2.0 * x.float())[~inf].to(F16))


def test_mixed_16bit_dtypes_are_an_error():
    from mine_amd.ops.backend import get_extension
    from mine_amd.ops.conv import pack_weights
    ext = get_extension(required=True)
    B, C, H, W, K = 1, 16, 8, 48, 16
    x = torch.zeros(B * H * W * C, device=DEV, dtype=F16)
    out = torch.empty(B * H * W * K, device=DEV, dtype=F16)
    wp = pack_weights(torch.zeros(K, C, 3, 3, device=DEV))
    assert wp.dtype == torch.bfloat16
    bias = torch.empty(0, device=DEV)
    with pytest.raises(RuntimeError):
        ext.conv3x3_fwd(x, wp, bias, out, B, H, W, C, K, 0, H, W, 0)
    ext.conv3x3_fwd(x, wp.to(F16), bias, out, B, H, W, C, K, 0, H, W, 0)
    assert not out.any()
