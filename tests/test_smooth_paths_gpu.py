"""Fused edge-aware smoothness v2 (loss_kernels.hip) on strided images,
unequal per-image means and exact ties.

Reference: the eager form of `edge_aware_loss_v2` on the CPU in fp64.
The first-round test passes a contiguous image only (the kernels take
four image strides), disparities whose per-image means are nearly equal
(so an error in the mean-normalisation term T_b hides), no exact ties
(sgn = 0) and bounds the gradient by atol 1e-5 against a median of
2.2e-4.

The tie case is a regression test: the backward used to take the sign of
`d0*inv_m - d1*inv_m`, which the compiler contracts to an FMA that
returns a rounding error instead of 0 at d0 == d1, so every tie got a
full-size gradient (error 9.2e-2 on a gradient of at most 1.3e-1 at
5x7). The kernels now difference the raw disparities.

Bound for the loss and for the gradient, as for SSIM:

    max(16 * dev32, 1e-5 * max|ref|)

with dev32 the largest deviation of the fp32 CPU eager path from the fp64
one on the same inputs.
"""
import functools

import pytest
import torch

from mine_amd.ops.losses import edge_aware_loss_v2

DEV = "cuda:0"
SHAPES = [(3, 5, 7), (2, 33, 47)]          # (B, H, W)
IMG_KINDS = ["contiguous", "channels_last", "crop"]
DISP_KINDS = ["scales", "ties"]
UPSTREAMS = [3.0, -0.5]
SCALES = {3: (0.1, 1.0, 10.0), 2: (0.1, 10.0)}
TIE = (slice(2, 10), slice(3, 11))         # the constant 8x8 block


def _img(shape, kind, device="cpu", dtype=torch.float32):
    """(B,3,H,W) image with the same values in every layout."""
    B, H, W = shape
    g = torch.Generator().manual_seed(300 + H)
    base = torch.rand(B, 3, H, W, generator=g).to(device=device, dtype=dtype)
    if kind == "contiguous":
        return base
    if kind == "channels_last":
        return base.contiguous(memory_format=torch.channels_last)
    big = torch.full((B, 3, H + 2, W + 5), 7.0, device=device, dtype=dtype)
    big[:, :, 1:-1, 2:-3] = base
    return big[:, :, 1:-1, 2:-3]


@functools.lru_cache(maxsize=None)
def _disp(shape, kind):
    B, H, W = shape
    g = torch.Generator().manual_seed(400 + H)
    d = torch.rand(B, 1, H, W, generator=g) * 2 + 0.1
    if kind == "scales":
        d = d * torch.tensor(SCALES[B]).view(B, 1, 1, 1)
    else:
        d[:, :, TIE[0], TIE[1]] = 0.75   # clipped by the 5x7 image
    return d.contiguous()


def _eager(shape, img_kind, disp_kind, upstream, dtype):
    d = _disp(shape, disp_kind).clone().to(dtype).requires_grad_(True)
    loss = edge_aware_loss_v2(_img(shape, img_kind, dtype=dtype), d)
    (loss * upstream).backward()
    return loss.detach().double(), d.grad.double()


@functools.lru_cache(maxsize=None)
def _reference(shape, disp_kind, upstream):
    """fp64 loss and gradient plus the fp32 eager deviations. The image
    layout does not change the values, so one reference serves all."""
    l64, g64 = _eager(shape, "contiguous", disp_kind, upstream, torch.float64)
    l32, g32 = _eager(shape, "contiguous", disp_kind, upstream, torch.float32)
    return dict(loss=l64, grad=g64, dev_loss=(l32 - l64).abs().item(),
                dev_grad=(g32 - g64).abs().max().item())


# ---------------------------------------------------------------------------
# CPU tests: the inputs are what the GPU tests take them for
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_image_layouts_hold_the_same_values_with_other_strides(shape):
    B, H, W = shape
    base = _img(shape, "contiguous")
    cl = _img(shape, "channels_last")
    crop = _img(shape, "crop")
    assert torch.equal(base, cl) and torch.equal(base, crop)
    assert base.stride() == (3 * H * W, H * W, W, 1)
    assert cl.stride() == (3 * H * W, 1, 3 * W, 3)
    assert crop.stride() == (3 * (H + 2) * (W + 5), (H + 2) * (W + 5),
                             W + 5, 1)
    assert crop.storage_offset() == (W + 5) + 2
    # every layout has a row stride other than W except the first, and
    # with W passed for it the reads stay inside the buffer
    assert cl.stride(2) > W and crop.stride(2) > W
    l0 = edge_aware_loss_v2(base.double(), _disp(shape, "scales").double())
    for other in (cl, crop):
        l1 = edge_aware_loss_v2(other.double(),
                                _disp(shape, "scales").double())
        assert abs(l0.item() - l1.item()) <= 1e-14 * abs(l0.item())


@pytest.mark.parametrize("shape", SHAPES)
def test_disparities_have_unequal_means_and_exact_ties(shape):
    B, H, W = shape
    means = _disp(shape, "scales").mean((1, 2, 3))
    assert (means.max() / means.min()).item() > 50.0
    d = _disp(shape, "ties")
    dx = d[:, :, :, 1:] - d[:, :, :, :-1]
    dy = d[:, :, 1:, :] - d[:, :, :-1, :]
    n_ties = int((dx == 0).sum() + (dy == 0).sum())
    rows, cols = min(H, 10) - 2, min(W, 11) - 3
    assert n_ties == B * (rows * (cols - 1) + (rows - 1) * cols) > 0
    # inside the block all four differences vanish: the eager gradient
    # there is the mean-normalisation term alone, one value per image
    ref = _reference(shape, "ties", 3.0)["grad"]
    if rows > 2 and cols > 2:
        inner = ref[:, 0, 3:min(H, 10) - 1, 4:min(W, 11) - 1]
        assert (inner.amax((1, 2)) - inner.amin((1, 2))).abs().max() \
            <= 1e-15
        assert inner.abs().min().item() > 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_eager_path_is_close_to_fp64(shape):
    for kind in DISP_KINDS:
        for up in UPSTREAMS:
            ref = _reference(shape, kind, up)
            gmax = ref["grad"].abs().max().item()
            print(f"eav2 {shape} {kind} up={up}: loss = "
                  f"{ref['loss'].item():.6f}, max|grad| = {gmax:.3e}, dev32 "
                  f"loss = {ref['dev_loss']:.2e}, grad = {ref['dev_grad']:.2e}")
            assert ref["dev_loss"] <= 1e-5 * abs(ref["loss"].item())
            assert ref["dev_grad"] <= 1e-4 * gmax


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

def _bound(dev32, ref):
    return max(16.0 * dev32, 1e-5 * ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("disp_kind", DISP_KINDS)
@pytest.mark.parametrize("img_kind", IMG_KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_eav2_fused_matches_fp64(shape, img_kind, disp_kind):
    img = _img(shape, img_kind, device=DEV)
    assert img.is_contiguous() == (img_kind == "contiguous")
    for up in UPSTREAMS:
        ref = _reference(shape, disp_kind, up)
        d = _disp(shape, disp_kind).clone().to(DEV).requires_grad_(True)
        loss = edge_aware_loss_v2(img, d)
        assert "EdgeAwareV2" in type(loss.grad_fn).__name__  # the HIP path
        (loss * up).backward()
        got_l = loss.detach().double().cpu()
        got_g = d.grad.double().cpu()
        assert bool(torch.isfinite(got_l)) and bool(torch.isfinite(got_g).all())
        b_l = _bound(ref["dev_loss"], ref["loss"])
        b_g = _bound(ref["dev_grad"], ref["grad"])
        e_l = (got_l - ref["loss"]).abs().item()
        e_g = (got_g - ref["grad"]).abs().max().item()
        print(f"eav2 {shape} {img_kind} {disp_kind} up={up}: loss err/bound "
              f"= {e_l / b_l:.3g} (err {e_l:.2e}, bound {b_l:.2e}); grad "
              f"err/bound = {e_g / b_g:.3g} (err {e_g:.2e}, bound {b_g:.2e})")
        assert e_l <= b_l
        assert e_g <= b_g
