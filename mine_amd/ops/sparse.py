"""Sparse-point gather (`gather_pixel_by_pxpy`), device-dispatched.

The eager form (`torch_ref.gather_pixel_by_pxpy`) is a `torch.gather`;
its backward on the GPU is an atomic scatter, and whenever two COLMAP
points round to one pixel — the normal case at the coarse scales — the
order of the adds, and with it the last bits of the disparity gradient,
changes from run to run. In deterministic mode on the GPU the op goes
through an autograd function whose backward is a HIP kernel without
atomics (`gather_pxpy_bwd_kernel`, loss_kernels.hip): the first point on
a pixel sums the gradients of all points on it in point order. The
forward is the same gather in both modes.
"""
from __future__ import annotations

import torch

from mine_amd.ops import torch_ref
from mine_amd.ops.backend import get_extension, is_deterministic


def _flat_index(pxpy: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Bx2xN pixel coordinates -> BxN flat indices, rounded and clamped as
    `torch_ref.gather_pixel_by_pxpy` does."""
    pp = torch.round(pxpy).to(torch.int64)
    px = torch.clamp(pp[:, 0], 0, W - 1)
    py = torch.clamp(pp[:, 1], 0, H - 1)
    return (px + W * py).contiguous()


class _GatherPxpyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, idx):
        B, C, H, W = img.shape
        ctx.save_for_backward(idx)
        ctx.geom = (H, W)
        return torch.gather(img.reshape(B, C, H * W), 2,
                            idx.unsqueeze(1).expand(B, C, idx.size(1)))

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        H, W = ctx.geom
        ext = get_extension(required=True)
        grad = ext.gather_pxpy_bwd(g.contiguous(), idx, H * W)
        return grad.view(g.shape[0], g.shape[1], H, W), None


def gather_pixel_by_pxpy(img: torch.Tensor, pxpy: torch.Tensor) -> torch.Tensor:
    """Round + clamp pixel coords, gather image values: BxCxHxW, Bx2xN ->
    BxCxN (ref operations/rendering_utils.py:27-44)."""
    if (img.is_cuda and img.dtype == torch.float32 and img.requires_grad
            and is_deterministic()):
        with torch.no_grad():
            idx = _flat_index(pxpy, img.shape[2], img.shape[3])
        return _GatherPxpyFn.apply(img, idx)
    return torch_ref.gather_pixel_by_pxpy(img, pxpy)
