"""The general igemm conv family (forward, data gradient, weight and bias
gradient) in fp16 on the seven shapes of
test_gpu_ops.py::test_conv_igemm_matches_torch, against fp64 CPU
references of the fp16-rounded inputs, at the derived bounds of
test_fp16_conv3x3_gpu.py rather than that test's 5e-2:
    forward        |y  - ref| <= 2^-10 * |ref| + 2^-13 * A
    data gradient  |gx - ref| <= (2^-10 + 2^-13) * A'
    weight grad    |dw - ref| <= M * 2^-24 * A'',  M = B*P*Q
    bias grad      rtol 1e-5, atol 1e-4 * sqrt(M)
A, A', A'' are the same sums over absolute values. The longest
contraction here is 9 * 128 = 1152 terms, 1152 * 2^-24 < 2^-13.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16 = torch.float16

SHAPES = [
    # (B, C, H, W, K, R, stride, pad, reflect)
    (4, 64, 16, 24, 256, 1, 1, 0, False),      # bottleneck 1x1
    (4, 256, 16, 24, 512, 1, 2, 0, False),     # downsample 1x1 s2
    (4, 64, 16, 24, 64, 3, 1, 1, False),       # bottleneck 3x3
    (4, 128, 16, 24, 128, 3, 2, 1, False),     # bottleneck 3x3 s2
    (2, 3, 32, 48, 64, 7, 2, 3, False),        # stem 7x7 s2 C=3 (pad8)
    (4, 96, 10, 14, 40, 3, 1, 1, True),        # reflect base conv
    (4, 24, 9, 13, 16, 1, 1, 0, False),        # odd sizes
]


def _conv(x, w, b, R, stride, pad, reflect):
    if reflect:
        p = (R - 1) // 2
        return F.conv2d(F.pad(x, (p,) * 4, mode="reflect"), w, b)
    return F.conv2d(x, w, b, stride=stride, padding=pad)


@functools.lru_cache(maxsize=None)
def _case(shape):
    B, C, H, W, K, R, stride, pad, reflect = shape
    g = torch.Generator().manual_seed(13)
    x = torch.randn(B, C, H, W, generator=g).to(F16)
    w = torch.randn(K, C, R, R, generator=g) * 0.2
    b = torch.randn(K, generator=g) * 0.1
    wq = w.to(F16).double()

    def run(xx, ww, bb, gg):
        xx = xx.requires_grad_(True)
        ww = ww.requires_grad_(True)
        y = _conv(xx, ww, bb, R, stride, pad, reflect)
        if gg is None:
            return y.detach()
        gx, gw = torch.autograd.grad(y, (xx, ww), gg)
        return y.detach(), gx, gw

    y0 = run(x.double(), wq.clone(), b.double(), None)
    gy = torch.randn(y0.shape, generator=g).to(F16)
    y, gx, gw = run(x.double(), wq.clone(), b.double(), gy.double())
    ya, gxa, gwa = run(x.double().abs(), wq.abs(), b.double().abs(),
                       gy.double().abs())
    return dict(x=x, w=w, b=b, gy=gy, y=y, y_abs=ya, gx=gx, gx_abs=gxa,
                gw=gw, gw_abs=gwa)


def _cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _within(err, bound, what):
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err > 0, torch.full_like(err, 2.0),
                                    torch.zeros_like(err)))
    worst = ratio.max().item()
    print(f"{what}: max err/bound {worst:.3f}")
    assert worst <= 1.0


def _run_gpu(shape):
    from mine_amd.ops.conv_general import conv2d_mfma
    B, C, H, W, K, R, stride, pad, reflect = shape
    c = _case(shape)
    x = _cl(c["x"]).requires_grad_(True)
    w = c["w"].to(DEV).requires_grad_(True)
    b = c["b"].to(DEV).requires_grad_(True)
    y = conv2d_mfma(x, w, b, stride=stride, padding=pad, reflect=reflect)
    y.backward(_cl(c["gy"]))
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("shape", SHAPES)
def test_igemm_fp16(shape):
    c = _case(shape)
    y, gx, gw, gb = _run_gpu(shape)
    assert y.dtype == F16 and gx.dtype == F16
    assert gw.dtype == torch.float32 and gb.dtype == torch.float32
    _within((y.double().cpu() - c["y"]).abs(),
            2.0 ** -10 * c["y"].abs() + 2.0 ** -13 * c["y_abs"], "fwd")
    _within((gx.double().cpu() - c["gx"]).abs(),
            (2.0 ** -10 + 2.0 ** -13) * c["gx_abs"], "dx")
    M = c["y"].numel() // c["y"].shape[1]
    _within((gw.double().cpu() - c["gw"]).abs(),
            M * 2.0 ** -24 * c["gw_abs"], "dw")
    ref = c["gy"].double().sum((0, 2, 3)).float()
    print(f"db: max abs err {(gb.cpu() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(gb.cpu(), ref, rtol=1e-5, atol=1e-4 * M ** 0.5)


def test_split_k_is_deterministic_in_fp16():
    """The batch-4 256-channel 1x1: its data gradient contracts over 512
    channels at M = 1536 pixels and takes the split-K path, its weight
    gradient the per-slab workspace."""
    from mine_amd.ops import deterministic
    shape = SHAPES[1]
    with deterministic():
        a = _run_gpu(shape)
        b = _run_gpu(shape)
    for name, p, q in zip(("y", "dx", "dw"), a, b):
        assert torch.equal(p, q), name
