"""Fused SSIM kernels at shapes that are no multiple of the 32x8 tile.

Reference: the project's eager path `ssim(..., force_torch=True)` on the
CPU in fp64. The first-round tests compare with the fp32 torch path on
the GPU at 64x96 and 48x64 only (tile multiples), with an atol of 1e-4
on a gradient whose largest entry is 1.3e-3.

Shapes (B,C,H,W): one exact tile (8x32), one pixel more than a tile in
both directions (9x33), partial tiles in both directions (13x45), the
flagship's smallest scale (32x48, half a tile in x) and an image smaller
than the 11-tap window (5x7).

Bound for the loss and for the gradient:

    max(16 * dev32, 1e-5 * max|ref|)

where dev32 is the largest deviation of the fp32 CPU eager path from the
fp64 one on the same inputs: the kernel sums the same 121 products per
moment in another order and forms S11 - mu1^2 like the eager path does,
so it may differ from fp64 by a small multiple of what fp32 eager does.

Identical pair, gradient only: the exact gradient is zero (SSIM(a, a) = 1
is the maximum), so max|ref| ~ 1e-17, and the eager fp32 backward happens
to cancel to a few 1e-9 or, at 8x32, to exactly 0: the formula above then
asks for a bit-exact zero. The kernel evaluates

    g/N * (blur(F1) + 2*img1*blur(F2) + img2*blur(F3))

whose three terms are O(10) each and cancel. Its floor for this input is
a first-order rounding bound, computed in fp64 from the inputs alone by
`_rounding_floor`: 22 FMA roundings per blurred moment, carried through
the cancelling differences S - mu^2 and S12 - mu1*mu2, the field
formulas, the 22 FMAs of the field blurs and the combine (details at
`_analytic`). `test_field_formulas_match_autograd` checks that the
expression itself is the gradient and that this worst-case floor stays
below 1e-3 of the random pair's largest gradient entry, the level the
identical pair's gradient has to stay under anyway.
"""
import functools

import pytest
import torch

from mine_amd.ops.ssim import ssim

DEV = "cuda:0"
UPSTREAM = -3.0
TW, TH, WINDOW = 32, 8, 11   # tile of ssim_kernels.hip, window taps

SHAPES = [(1, 3, 8, 32), (1, 2, 9, 33), (2, 3, 13, 45), (2, 3, 32, 48),
          (1, 1, 5, 7)]
KINDS = ["random", "identical", "constant", "channels_last"]


@functools.lru_cache(maxsize=None)
def _pair(shape, kind):
    """fp32 CPU (img1, img2)."""
    g = torch.Generator().manual_seed(1000 + 17 * SHAPES.index(shape))
    a = torch.rand(*shape, generator=g)
    b = torch.rand(*shape, generator=g)
    if kind == "identical":
        b = a.clone()
    elif kind == "constant":
        a = torch.full(shape, 0.3)
        b = torch.full(shape, 0.7)
    elif kind == "channels_last":
        a = a.contiguous(memory_format=torch.channels_last)
    return a, b


def _eager(a, b, dtype):
    a = a.detach().to(dtype).requires_grad_(True)
    val = ssim(a, b.to(dtype), force_torch=True)
    (val * UPSTREAM).backward()
    return val.detach().double(), a.grad.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, kind):
    """fp64 value and gradient, and the fp32 eager path's deviation."""
    a, b = _pair(shape, kind)
    v64, g64 = _eager(a, b, torch.float64)
    v32, g32 = _eager(a, b, torch.float32)
    return dict(val=v64, grad=g64,
                dev_val=(v32 - v64).abs().item(),
                dev_grad=(g32 - g64).abs().max().item())


_U = 2.0 ** -24   # fp32 unit roundoff


def _analytic(a, b):
    """The backward kernels' expression in fp64, with a first-order bound
    on its fp32 rounding error: (gradient, per-pixel error bound).

    Every blurred moment carries 22 FMA roundings plus the square or
    product under it: relative error um = 24u. From there
      dA1 = 2um*A1, dB1 = 2um*B1,
      dA2 = 2um*A2m, dB2 = 2um*B2m
    with A2m, B2m the sums of the magnitudes of the operands of the
    cancelling differences S12 - mu1*mu2 and S - mu^2; the errors go
    through the field formulas by the product rule (a few u more for the
    formulas' own operations), through the second blur (22u of the
    blurred magnitude) and through the combine (5u)."""
    from mine_amd.ops.ssim import _C1, _C2, _blur, _window
    a, b = a.double().contiguous(), b.double().contiguous()
    w = _window(a.device, a.dtype)
    mu1, mu2 = _blur(a, w), _blur(b, w)
    S11, S22, S12 = _blur(a * a, w), _blur(b * b, w), _blur(a * b, w)
    A1 = 2 * mu1 * mu2 + _C1
    A2 = 2 * (S12 - mu1 * mu2) + _C2
    B1 = mu1 * mu1 + mu2 * mu2 + _C1
    B2 = (S11 - mu1 * mu1) + (S22 - mu2 * mu2) + _C2
    iB = 1.0 / (B1 * B2)
    f1a = 2 * mu2 * (A2 - A1) * iB
    f1b = 2 * mu1 * A1 * A2 * (B1 - B2) * iB * iB
    f2 = -A1 * A2 * B1 * iB * iB
    f3 = 2 * A1 * iB
    scale = UPSTREAM / a.numel()
    grad = scale * (_blur(f1a + f1b, w) + 2 * a * _blur(f2, w) +
                    b * _blur(f3, w))

    um = 24 * _U
    dA1, dB1 = 2 * um * A1.abs(), 2 * um * B1
    dA2 = 2 * um * (2 * (S12 + (mu1 * mu2).abs()) + _C2)
    dB2 = 2 * um * ((S11 + mu1 * mu1) + (S22 + mu2 * mu2) + _C2)
    rB = dB1 / B1 + dB2 / B2          # relative error of B1*B2
    d3 = 2 * dA1 * iB + f3.abs() * (rB + 4 * _U)
    d2 = (dA1 * A2.abs() + A1.abs() * dA2) * B1 * iB * iB + \
        f2.abs() * (dB1 / B1 + 2 * rB + 6 * _U)
    d1a = 2 * mu2.abs() * (dA2 + dA1) * iB + f1a.abs() * (um + rB + 4 * _U)
    d1b = 2 * mu1.abs() * iB * iB * (
        (dA1 * A2.abs() + A1.abs() * dA2) * (B1 - B2).abs() +
        (A1 * A2).abs() * (dB1 + dB2)) + \
        f1b.abs() * (um + 2 * rB + 8 * _U)
    blur_err = lambda d, f: _blur(d + 22 * _U * f.abs(), w)
    e1 = blur_err(d1a + d1b, f1a.abs() + f1b.abs())
    e2 = blur_err(d2, f2)
    e3 = blur_err(d3, f3)
    m1, m2, m3 = (_blur(f.abs(), w) for f in (f1a.abs() + f1b.abs(), f2, f3))
    err = abs(scale) * (e1 + 2 * a.abs() * e2 + b.abs() * e3 +
                        5 * _U * (m1 + 2 * a.abs() * m2 + b.abs() * m3))
    return grad, err


def _rounding_floor(shape, kind):
    a, b = _pair(shape, kind)
    _, err = _analytic(a, b)
    return err.max().item()


def _fused(shape, kind):
    a, b = _pair(shape, kind)
    a = a.to(DEV).requires_grad_(True)
    if kind == "channels_last" and 1 not in shape[:2]:
        assert not a.is_contiguous()
    val = ssim(a, b.to(DEV))
    assert "SsimFn" in type(val.grad_fn).__name__  # the HIP path
    (val * UPSTREAM).backward()
    return val.detach().double().cpu(), a.grad.double().cpu()


# ---------------------------------------------------------------------------
# CPU tests: the inputs are what the GPU tests take them for
# ---------------------------------------------------------------------------

def test_shapes_cover_the_tile_edges():
    part_x = [s for s in SHAPES if s[3] % TW]
    part_y = [s for s in SHAPES if s[2] % TH]
    exact = [s for s in SHAPES if s[3] % TW == 0 and s[2] % TH == 0]
    multi = [s for s in SHAPES if s[3] > TW and s[2] > TH]
    small = [s for s in SHAPES if s[3] < WINDOW and s[2] < WINDOW]
    assert part_x and part_y and exact and multi and small
    assert (2, 3, 32, 48) in SHAPES  # smallest flagship scale
    # one pixel past the tile in both directions
    assert any(s[3] == TW + 1 and s[2] == TH + 1 for s in SHAPES)


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_eager_path_is_close_to_fp64(shape):
    """dev32 is a rounding-level quantity, so 16*dev32 is a tight bound."""
    for kind in KINDS:
        ref = _reference(shape, kind)
        print(f"ssim {shape} {kind}: val = {ref['val'].item():.6f}, "
              f"max|grad| = {ref['grad'].abs().max().item():.3e}, dev32 val = "
              f"{ref['dev_val']:.2e}, grad = {ref['dev_grad']:.2e}")
        assert ref["dev_val"] <= 1e-5
        assert ref["dev_grad"] <= 1e-3 * \
            _reference(shape, "random")["grad"].abs().max().item()


@pytest.mark.parametrize("shape", SHAPES)
def test_special_pairs_are_special(shape):
    ident = _reference(shape, "identical")
    rand = _reference(shape, "random")
    const = _reference(shape, "constant")
    # SSIM(a, a) = 1 is the maximum: value 1, gradient 0 in exact arithmetic
    assert abs(ident["val"].item() - 1.0) < 1e-12
    assert ident["grad"].abs().max().item() <= \
        1e-9 * rand["grad"].abs().max().item()
    # constant images: zero variance away from the zero-padded border
    a, b = _pair(shape, "constant")
    assert float(a.min()) == float(a.max()) == pytest.approx(0.3)
    assert float(b.min()) == float(b.max()) == pytest.approx(0.7)
    assert 0.0 < const["val"].item() < 1.0
    a, _ = _pair(shape, "channels_last")
    if 1 not in shape[:2]:
        assert not a.is_contiguous()
        assert a.is_contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("shape", SHAPES)
def test_field_formulas_match_autograd(shape):
    """The expression behind `_rounding_floor` is the gradient, and the
    floor it gives for the identical pair is far below the signal."""
    for kind in ("random", "constant"):
        a, b = _pair(shape, kind)
        grad, err = _analytic(a, b)
        ref = _reference(shape, kind)["grad"]
        assert (grad - ref).abs().max().item() <= \
            1e-10 * ref.abs().max().item()
        assert bool((err > 0).all())
    floor = _rounding_floor(shape, "identical")
    signal = _reference(shape, "random")["grad"].abs().max().item()
    print(f"ssim {shape}: identical-pair floor = {floor:.2e} = "
          f"{floor / signal:.2e} of the random pair's max|grad|")
    assert floor <= 1e-3 * signal


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

def _bound(dev32, ref):
    return max(16.0 * dev32, 1e-5 * ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_fused_matches_fp64(shape, kind):
    ref = _reference(shape, kind)
    val, grad = _fused(shape, kind)
    assert grad.shape == ref["grad"].shape
    assert bool(torch.isfinite(val)) and bool(torch.isfinite(grad).all())
    b_val = _bound(ref["dev_val"], ref["val"])
    b_grad = _bound(ref["dev_grad"], ref["grad"])
    if kind == "identical":   # zero reference: see the module docstring
        b_grad = max(b_grad, _rounding_floor(shape, kind))
    e_val = (val - ref["val"]).abs().item()
    e_grad = (grad - ref["grad"]).abs().max().item()
    print(f"ssim {shape} {kind}: value err/bound = {e_val / b_val:.3g} "
          f"(err {e_val:.2e}, bound {b_val:.2e}); grad err/bound = "
          f"{e_grad / b_grad:.3g} (err {e_grad:.2e}, bound {b_grad:.2e})")
    assert e_val <= b_val
    assert e_grad <= b_grad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_ssim_identical_pair_gradient_vanishes(shape):
    _, g_ident = _fused(shape, "identical")
    _, g_rand = _fused(shape, "random")
    ratio = g_ident.abs().max().item() / g_rand.abs().max().item()
    print(f"ssim {shape}: max|grad identical| / max|grad random| = "
          f"{ratio:.3g}")
    assert ratio < 1e-3
