"""Reflection pad, nearest x2 upsample and the MPI head pack in fp16.

The forwards of pad and upsample are copies and must equal torch's result
bit for bit. Their backwards sum up to 9 (pad) or exactly 4 (upsample)
fp16 terms in fp32 and round once: |err| <= 2^-10 * sum|terms| (the
half-ulp 2^-11 with a factor 2, as for the convolutions). Shapes are
those of the bf16 tests in test_gpu_ops.py. The head pack computes in
fp32 and writes fp32, so it is held to that test's fp32 tolerance against
the fp32 path fed the same fp16-rounded input.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16 = torch.float16


def _within(got, ref, ref_abs):
    err = (got.double().cpu() - ref).abs()
    bound = 2.0 ** -10 * ref_abs
    worst = (err / bound.clamp_min(1e-30)).max().item()
    print(f"max err/bound {worst:.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("pad", [1, 2])
def test_reflection_pad(channels_last, pad):
    from mine_amd.ops.pad import reflection_pad2d
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(3, 7, 10, 14, generator=g).to(F16)
    gy0 = torch.randn(3, 7, 10 + 2 * pad, 14 + 2 * pad, generator=g).to(F16)
    x = x0.to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    x = x.requires_grad_(True)
    y = reflection_pad2d(x, pad)
    assert y.dtype == F16
    assert torch.equal(y.cpu(), F.pad(x0, (pad,) * 4, mode="reflect"))
    y.backward(gy0.to(DEV))

    def fold(gg):
        xr = torch.zeros(x0.shape, dtype=torch.float64, requires_grad=True)
        F.pad(xr, (pad,) * 4, mode="reflect").backward(gg)
        return xr.grad
    _within(x.grad, fold(gy0.double()), fold(gy0.double().abs()))


def test_reflection_pad_vector_path():
    """C % 8 == 0 channels_last: one 16-byte vector per thread."""
    from mine_amd.ops.pad import reflection_pad2d
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(2, 16, 6, 9, generator=g).to(F16)
    x = x0.to(DEV).contiguous(memory_format=torch.channels_last)
    assert torch.equal(reflection_pad2d(x, 1).cpu(),
                       F.pad(x0, (1, 1, 1, 1), mode="reflect"))


def test_upsample2x():
    from mine_amd.ops.upsample import upsample_nearest2x
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(3, 16, 9, 26, generator=g).to(F16)
    gy0 = torch.randn(3, 16, 18, 52, generator=g).to(F16)
    x = x0.to(DEV).contiguous(memory_format=torch.channels_last
                              ).requires_grad_(True)
    y = upsample_nearest2x(x)
    assert y.shape == (3, 16, 18, 52) and y.dtype == F16
    assert torch.equal(y.cpu(), F.interpolate(x0, scale_factor=2,
                                              mode="nearest"))
    y.backward(gy0.to(DEV))
    pool = lambda t: F.avg_pool2d(t, 2) * 4.0  # noqa: E731  sum of 4 children
    _within(x.grad, pool(gy0.double()), pool(gy0.double().abs()))


@pytest.mark.parametrize("use_alpha", [False, True])
def test_mpi_head_pack(use_alpha):
    from mine_amd.ops.head import mpi_head_pack
    g = torch.Generator().manual_seed(21)
    B, S, H, W = 2, 6, 13, 19
    z0 = (torch.randn(B * S, 4, H, W, generator=g) * 2.0).to(F16)
    gw = torch.randn(B, S, H, W, 4, generator=g).to(DEV)

    def run(dtype):
        z = z0.to(DEV, dtype).contiguous(memory_format=torch.channels_last
                                         ).requires_grad_(True)
        out = mpi_head_pack(z, B, S, use_alpha)
        assert out.dtype == torch.float32 and out.shape == (B, S, H, W, 4)
        (out * gw).sum().backward()
        return out.detach(), z.grad

    out16, gz16 = run(F16)
    out32, gz32 = run(torch.float32)
    assert gz16.dtype == F16
    tol = dict(rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out16, out32, **tol)
    # the gradient is stored in fp16: compare with the fp32 path's
    # gradient rounded the same way
    torch.testing.assert_close(gz16.float(), gz32.to(F16).float(),
                               rtol=2.0 ** -10, atol=2.0 ** -24)
