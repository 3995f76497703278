"""SSIM with an 11x11 sigma=1.5 Gaussian window (ref network/ssim.py).

Torch path: 5 depthwise conv2d with a separable window (the reference
used a full 2D 11x11 kernel; separable halves the work at identical
numerics since the window is an outer product). On CUDA, a fused HIP
kernel computes all five windowed moments in one pass (forward) and the
analytic gradient w.r.t. img1 in two passes (backward).
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from mine_amd.ops.backend import get_extension, is_deterministic

_C1 = 0.01 ** 2
_C2 = 0.03 ** 2
_WINDOW_SIZE = 11
_SIGMA = 1.5


def gaussian_window_1d(size: int = _WINDOW_SIZE, sigma: float = _SIGMA) -> torch.Tensor:
    g = torch.tensor([math.exp(-((x - size // 2) ** 2) / (2.0 * sigma ** 2))
                      for x in range(size)])
    return g / g.sum()


_win_cache: Dict[Tuple[torch.device, torch.dtype], torch.Tensor] = {}


def _window(device, dtype) -> torch.Tensor:
    key = (device, dtype)
    w = _win_cache.get(key)
    if w is None:
        w = gaussian_window_1d().to(device=device, dtype=dtype)
        _win_cache[key] = w
    return w


def _blur(x: torch.Tensor, w1d: torch.Tensor) -> torch.Tensor:
    """Separable depthwise Gaussian blur with zero padding (matches the
    reference's F.conv2d(padding=5) on a 2D outer-product window)."""
    B, C, H, W = x.shape
    pad = _WINDOW_SIZE // 2
    kh = w1d.view(1, 1, _WINDOW_SIZE, 1).expand(C, 1, _WINDOW_SIZE, 1)
    kw = w1d.view(1, 1, 1, _WINDOW_SIZE).expand(C, 1, 1, _WINDOW_SIZE)
    x = F.conv2d(x, kw, padding=(0, pad), groups=C)
    x = F.conv2d(x, kh, padding=(pad, 0), groups=C)
    return x


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        ext = get_extension(required=True)
        # deterministic mode: per-block partials summed in a fixed order
        # instead of one atomic per block (the backward has no reduction)
        mean, = ext.ssim_fwd(img1, img2, is_deterministic())
        ctx.save_for_backward(img1, img2)
        return mean

    @staticmethod
    def backward(ctx, g):
        img1, img2 = ctx.saved_tensors
        ext = get_extension(required=True)
        grad1 = ext.ssim_bwd(img1, img2, g.contiguous())
        return grad1, None


def ssim(img1: torch.Tensor, img2: torch.Tensor, size_average: bool = True,
         force_torch: bool = False) -> torch.Tensor:
    """Mean SSIM over the batch. img1 carries gradient; img2 is treated as
    ground truth (matching how the reference uses it: 1 - ssim(syn, gt))."""
    if img1.is_cuda and size_average and not force_torch:
        return _SsimFn.apply(img1.contiguous(), img2.detach().contiguous())

    w = _window(img1.device, img1.dtype)
    mu1 = _blur(img1, w)
    mu2 = _blur(img2, w)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sigma1_sq = _blur(img1 * img1, w) - mu1_sq
    sigma2_sq = _blur(img2 * img2, w) - mu2_sq
    sigma12 = _blur(img1 * img2, w) - mu1_mu2

    ssim_map = ((2 * mu1_mu2 + _C1) * (2 * sigma12 + _C2)) / \
               ((mu1_sq + mu2_sq + _C1) * (sigma1_sq + sigma2_sq + _C2))
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)
