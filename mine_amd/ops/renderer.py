"""High-level differentiable MPI rendering, device-dispatched.

The MPI travels through this module PACKED as (B, S, H, W, 4) — rgb and
sigma adjacent per pixel — which is the layout the CDNA4 kernels consume
with single float4/bf16x4 gathers (and what a channels_last decoder head
produces with a zero-copy permute). The reference instead materialized
nine BxSx{3,1,7}xHxW intermediates per scale (xyz src/tgt, 7-ch concat,
warped stack, transparency, weights...; ref operations/
mpi_rendering.py:181-241); here the source composite is ONE fused kernel
and the novel-view render is ONE fused kernel that loops the S planes
in-register per output pixel.

Fused op 1 — render_src_view:
    per pixel: delta_s = |K^-1 p| * (d_{s+1}-d_s) (far plane 1e3),
    t = exp(-sigma*delta), A = shifted-cumprod(t+1e-6), w = A*(1-t),
    optional RGB blending c = A*I + (1-A)*rgb (ref synthesis_task.py:267-274),
    outputs composited rgb/depth and the blended MPI for the tgt warp.

Fused op 2 — render_tgt_view:
    per tgt pixel, loop s: project through per-plane H_src_tgt (closed-form
    inverse homography), border-clamp, bilinear-gather rgb+sigma (float4),
    compute the warped plane point analytically (bilinear sampling of a
    linear field == evaluation at the mapped point), z-cull, and
    volume-composite — no warped stack is ever materialized.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from mine_amd.ops import torch_ref as tr
from mine_amd.ops.backend import get_extension, is_deterministic

_TGT_BWD_MODE = None


def tgt_bwd_mode() -> int:
    """1 (default) = gather-based warp backward (per-src-tile inversion,
    no interior atomics); 0 = the round-1 all-atomic bilinear scatter.
    Override with MINE_TGT_BWD=scatter. Deterministic mode runs mode 2
    (order-fixed emit + collect) whatever this returns."""
    global _TGT_BWD_MODE
    if _TGT_BWD_MODE is None:
        import os
        _TGT_BWD_MODE = 0 if os.environ.get("MINE_TGT_BWD") == "scatter" else 1
    return _TGT_BWD_MODE


# ---------------------------------------------------------------------------
# packing helpers
# ---------------------------------------------------------------------------


def pack_mpi(rgb: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """BxSx3xHxW + BxSx1xHxW -> BxSxHxWx4 contiguous."""
    return torch.cat((rgb, sigma), dim=2).permute(0, 1, 3, 4, 2).contiguous()


def unpack_mpi(mpi: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """BxSxHxWx4 -> (BxSx3xHxW, BxSx1xHxW) views."""
    chan_first = mpi.permute(0, 1, 4, 2, 3)
    return chan_first[:, :, 0:3], chan_first[:, :, 3:4]


def _img_packed(img: torch.Tensor) -> torch.Tensor:
    """Bx3xHxW (any layout) -> BxHxWx3 contiguous."""
    return img.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------
# source-view composite (+ RGB blending), fused on GPU
# ---------------------------------------------------------------------------


class _SrcCompositeFn(torch.autograd.Function):
    """Fused src-view volume composite + RGB blending.

    inputs:  mpi (B,S,H,W,4) float32, depths (B,S) fp32 ascending,
             K_inv (B,3,3) fp32, src_img (B,H,W,3) fp32 or empty,
             bg_depth_inf flag
    outputs: rgb_syn (B,3,H,W), depth_syn (B,1,H,W), mpi_blend (B,S,H,W,4)
    """

    @staticmethod
    def forward(ctx, mpi, depths, k_inv, src_img, bg_inf, blend, alpha):
        ext = get_extension(required=True)
        rgb_syn, depth_syn, mpi_blend = ext.src_composite_fwd(
            mpi, depths, k_inv,
            src_img if blend else torch.empty(0, device=mpi.device, dtype=mpi.dtype),
            bool(bg_inf), bool(alpha))
        ctx.save_for_backward(mpi, depths, k_inv, src_img)
        ctx.bg_inf = bool(bg_inf)
        ctx.blend = bool(blend)
        ctx.alpha = bool(alpha)
        return rgb_syn, depth_syn, mpi_blend

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_blend):
        mpi, depths, k_inv, src_img = ctx.saved_tensors
        ext = get_extension(required=True)
        empty = torch.empty(0, device=mpi.device, dtype=mpi.dtype)
        grad_mpi = ext.src_composite_bwd(
            mpi, depths, k_inv,
            src_img if ctx.blend else empty,
            ctx.bg_inf, ctx.alpha,
            g_rgb.contiguous() if g_rgb is not None else empty,
            g_depth.contiguous() if g_depth is not None else empty,
            g_blend.contiguous() if (ctx.blend and g_blend is not None) else empty)
        return grad_mpi, None, None, None, None, None, None


def render_src_view(mpi: torch.Tensor,
                    disparity: torch.Tensor,
                    K_inv: torch.Tensor,
                    src_img: Optional[torch.Tensor] = None,
                    bg_depth_inf: bool = False,
                    use_alpha: bool = False,
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Composite the MPI in the source camera.

    mpi: (B,S,H,W,4) packed rgb+sigma; disparity: (B,S) descending;
    K_inv: (B,3,3); src_img: (B,3,H,W) to enable RGB blending
    (ref synthesis_task.py:260-274).

    Returns (rgb_syn (B,3,H,W), depth_syn (B,1,H,W),
             mpi_blend (B,S,H,W,4) — input mpi with blended rgb; equals
             `mpi` when src_img is None).
    """
    blend = (src_img is not None) and not use_alpha
    if mpi.is_cuda:
        # alpha mode: no RGB blending, no background term
        # (ref mpi_rendering.py:19-39)
        depths = torch.reciprocal(disparity).to(torch.float32)
        img_p = _img_packed(src_img.to(torch.float32)) if blend \
            else torch.empty(0, device=mpi.device)
        out = _SrcCompositeFn.apply(mpi.contiguous(), depths.contiguous(),
                                    K_inv.to(torch.float32).contiguous(),
                                    img_p, bg_depth_inf, blend, use_alpha)
        if use_alpha:
            return out[0], out[1], mpi
        return out

    # -------- torch reference path (CPU, and the use_alpha branch) --------
    rgb, sigma = unpack_mpi(mpi)
    grid = tr.make_meshgrid(mpi.shape[2], mpi.shape[3], device=mpi.device)
    xyz = tr.src_plane_xyz(grid, disparity, K_inv)
    if use_alpha:
        # no RGB blending under alpha compositing (ref mpi_rendering.py:19)
        rgb_syn, _ = tr.alpha_composite(sigma, rgb)
        depth_syn, _ = tr.alpha_composite(sigma, xyz[:, :, 2:])
        return rgb_syn, depth_syn, mpi
    rgb_syn, depth_syn, acc, weights = tr.volume_composite(rgb, sigma, xyz, bg_depth_inf)
    if blend:
        blended = acc * src_img.unsqueeze(1) + (1.0 - acc) * rgb
        rgb_syn, depth_syn = tr.weighted_sum_mpi(blended, xyz, weights, bg_depth_inf)
        mpi_blend = pack_mpi(blended, sigma)
    else:
        mpi_blend = mpi
    return rgb_syn, depth_syn, mpi_blend


# ---------------------------------------------------------------------------
# novel-view render, fused on GPU
# ---------------------------------------------------------------------------


class _TgtCompositeFn(torch.autograd.Function):
    """Fused homography warp + z-cull + volume composite.

    inputs:  mpi (B,S,H,W,4), hinv (B,S,3,3) = H_src_tgt per plane,
             m (B,3,3) = R_tgt_src @ K_src_inv, tvec (B,3), depths (B,S)
    outputs: tgt_rgb (B,3,H,W), tgt_depth (B,1,H,W), tgt_mask (B,1,H,W)
    """

    @staticmethod
    def forward(ctx, mpi, hinv, m, tvec, depths, bg_inf, alpha):
        ext = get_extension(required=True)
        rgb, depth, mask = ext.tgt_composite_fwd(mpi, hinv, m, tvec, depths,
                                                 bool(bg_inf), bool(alpha))
        ctx.save_for_backward(mpi, hinv, m, tvec, depths)
        ctx.bg_inf = bool(bg_inf)
        ctx.alpha = bool(alpha)
        # read once here (as ops/bn.py does): a graph built in
        # deterministic mode keeps the order-fixed backward
        ctx.det = is_deterministic()
        return rgb, depth, mask

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_mask):
        mpi, hinv, m, tvec, depths = ctx.saved_tensors
        ext = get_extension(required=True)
        empty = torch.empty(0, device=mpi.device, dtype=torch.float32)
        # mode 2 (order-fixed emit + collect, no float atomics) overrides
        # MINE_TGT_BWD in deterministic mode
        mode = 2 if ctx.det else tgt_bwd_mode()
        if mode >= 1:
            # gather / collect: inverting the map per source tile or texel
            # needs the forward (src -> tgt pixel) homographies
            from mine_amd.utils.geometry import inverse_3x3
            with torch.no_grad():
                B, S = hinv.shape[0], hinv.shape[1]
                hfwd = inverse_3x3(hinv.reshape(B * S, 3, 3)) \
                    .reshape(B, S, 3, 3).contiguous()
        else:
            hfwd = empty
        grad_mpi = ext.tgt_composite_bwd(
            mpi, hinv, hfwd, m, tvec, depths, ctx.bg_inf, ctx.alpha,
            g_rgb.contiguous() if g_rgb is not None else empty,
            g_depth.contiguous() if g_depth is not None else empty,
            mode)
        return grad_mpi, None, None, None, None, None, None


class _TgtViewsFn(torch.autograd.Function):
    """_TgtCompositeFn for V cameras that read ONE MPI.

    inputs:  mpi (B,S,H,W,4), hinv (V,B,S,3,3), m (V,B,3,3), tvec (V,B,3),
             depths (B,S)
    outputs: tgt_rgb (V,B,3,H,W), tgt_depth (V,B,1,H,W), tgt_mask (V,B,1,H,W)

    The forward is one launch of the single-view kernel over V*B view
    rows. The backward leaves ONE grad_mpi through ONE MPI-sized payload,
    view after view in stream order.
    """

    @staticmethod
    def forward(ctx, mpi, hinv, m, tvec, depths, bg_inf, alpha):
        ext = get_extension(required=True)
        V = hinv.shape[0]
        rgb, depth, mask = ext._views.tgt_views_fwd(
            mpi, hinv, m, tvec, depths, V, bool(bg_inf), bool(alpha))
        ctx.save_for_backward(mpi, hinv, m, tvec, depths)
        ctx.bg_inf = bool(bg_inf)
        ctx.alpha = bool(alpha)
        # read once here, as _TgtCompositeFn does
        ctx.det = is_deterministic()
        return rgb, depth, mask

    @staticmethod
    def backward(ctx, g_rgb, g_depth, g_mask):
        mpi, hinv, m, tvec, depths = ctx.saved_tensors
        ext = get_extension(required=True)
        empty = torch.empty(0, device=mpi.device, dtype=torch.float32)
        mode = 2 if ctx.det else tgt_bwd_mode()
        if mode >= 1:
            from mine_amd.utils.geometry import inverse_3x3
            with torch.no_grad():
                hfwd = inverse_3x3(hinv.reshape(-1, 3, 3)) \
                    .reshape(hinv.shape).contiguous()
        else:
            hfwd = empty
        grad_mpi = ext._views.tgt_views_bwd(
            mpi, hinv, hfwd, m, tvec, depths, hinv.shape[0], ctx.bg_inf,
            ctx.alpha,
            g_rgb.contiguous() if g_rgb is not None else empty,
            g_depth.contiguous() if g_depth is not None else empty,
            mode)
        return grad_mpi, None, None, None, None, None, None


def render_tgt_views(mpi: torch.Tensor,
                     disparity: torch.Tensor,
                     G_tgt_src: torch.Tensor,
                     K_src_inv: torch.Tensor,
                     K_tgt: torch.Tensor,
                     bg_depth_inf: bool = False,
                     use_alpha: bool = False,
                     ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Render ONE MPI into V novel views.

    mpi (B,S,H,W,4), disparity (B,S) and K_src_inv (B,3,3) as in
    render_tgt_view; G_tgt_src (V,B,4,4) and K_tgt (V,B,3,3) are
    view-major. Returns (tgt_rgb (V,B,3,H,W), tgt_depth (V,B,1,H,W),
    tgt_mask (V,B,1,H,W)): every [v] slice is what render_tgt_view gives
    for view v, bit for bit on the GPU. Differentiable in mpi only; its
    gradient is the sum over the views, accumulated in one MPI-sized
    buffer (no per-view copy of the MPI or of its gradient).
    """
    V, B = G_tgt_src.shape[0], mpi.shape[0]
    if G_tgt_src.dim() != 4 or G_tgt_src.shape[1] != B \
            or K_tgt.shape[:2] != G_tgt_src.shape[:2]:
        raise ValueError(
            "render_tgt_views: G_tgt_src must be (V,B,4,4) and K_tgt "
            f"(V,B,3,3) with B = {B}, got {tuple(G_tgt_src.shape)} and "
            f"{tuple(K_tgt.shape)}")
    if mpi.is_cuda:
        depths = torch.reciprocal(disparity).to(torch.float32)
        with torch.no_grad():
            # all V*B*S planes in one batched call
            G = G_tgt_src.reshape(V * B, 4, 4)
            K_si = K_src_inv.repeat(V, 1, 1)
            hinv = tr.homography_tgt_to_src(
                G, depths.repeat(V, 1), K_si, K_tgt.reshape(V * B, 3, 3))
            S = depths.shape[1]
            hinv = hinv.reshape(V, B, S, 3, 3).contiguous()
            m = torch.matmul(G[:, :3, :3], K_si).reshape(V, B, 3, 3) \
                .contiguous()
            tvec = G[:, :3, 3].reshape(V, B, 3).contiguous()
        return _TgtViewsFn.apply(mpi.contiguous(), hinv, m, tvec,
                                 depths.contiguous(), bg_depth_inf, use_alpha)

    rgb, sigma = unpack_mpi(mpi)
    if V == 0:
        raise ValueError("render_tgt_views: needs at least one view")
    outs = [tr.render_tgt_reference(rgb, sigma, disparity, G_tgt_src[v],
                                    K_src_inv, K_tgt[v], use_alpha=use_alpha,
                                    bg_depth_inf=bg_depth_inf)
            for v in range(V)]
    return tuple(torch.stack(o, dim=0) for o in zip(*outs))


def render_tgt_view(mpi: torch.Tensor,
                    disparity: torch.Tensor,
                    G_tgt_src: torch.Tensor,
                    K_src_inv: torch.Tensor,
                    K_tgt: torch.Tensor,
                    bg_depth_inf: bool = False,
                    use_alpha: bool = False,
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Render the MPI into a novel view.

    mpi: (B,S,H,W,4) packed (blended) rgb+sigma; disparity (B,S) descending;
    G_tgt_src (B,4,4); K_src_inv/K_tgt (B,3,3).
    Returns (tgt_rgb (B,3,H,W), tgt_depth (B,1,H,W), tgt_mask (B,1,H,W)).
    Geometry inputs carry no gradient (poses/intrinsics are data; the
    scale-factored translation is detached upstream exactly as the
    reference does, ref synthesis_task.py:439-442).
    """
    depths = torch.reciprocal(disparity).to(torch.float32)
    if mpi.is_cuda:
        with torch.no_grad():
            hinv = tr.homography_tgt_to_src(G_tgt_src, depths, K_src_inv, K_tgt)
            m = torch.matmul(G_tgt_src[:, :3, :3], K_src_inv).contiguous()
            tvec = G_tgt_src[:, :3, 3].contiguous()
        return _TgtCompositeFn.apply(mpi.contiguous(), hinv.contiguous(), m, tvec,
                                     depths.contiguous(), bg_depth_inf,
                                     use_alpha)

    rgb, sigma = unpack_mpi(mpi)
    return tr.render_tgt_reference(rgb, sigma, disparity, G_tgt_src,
                                   K_src_inv, K_tgt, use_alpha=use_alpha,
                                   bg_depth_inf=bg_depth_inf)
