"""Fused BatchNorm + activation on the HIP kernels.

Training-mode BN with fp32 statistics over bf16, fp16 (or fp32) channels_last
activations, with the following activation fused into the normalize pass
(and its derivative into the backward): none / relu / lrelu(0.1) / elu /
add_relu (the ResNet residual join y = relu(bn(x) + res)).

Replaces the eager chain the profile showed as ~20% of the step
(cast->MIOpen BN->cast->activation, fwd+bwd; see
profiles/r01_flagship_kernel_stats.md). `FusedBNAct` subclasses
nn.BatchNorm2d so parameter/buffer names (weight, bias, running_mean,
running_var, num_batches_tracked) — and therefore the checkpoint
contract — are unchanged (ref CS5).

Small layers (the batch-4 encoder and neck; `ext._bn.small_plan`) take a
two-launch path per direction: a reduction into a few partial rows and a
consumer that finishes the sum in its prologue and also does the finalize,
the running-statistics update and the batch count. It is order-fixed, so
it serves the default and the deterministic mode alike; MINE_BN_COMPACT=0
turns it off.

Fallback paths (CPU, non-channels_last, exotic dtype, eval-with-grad):
fp32 functional BN + eager activation, numerically equivalent.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from mine_amd.ops.backend import get_extension, is_deterministic

_ACT = {"none": 0, "relu": 1, "lrelu": 2, "elu": 3, "add_relu": 4}


class _BNActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_flat, res_flat, mean, invstd, gamma, beta, M, C, act,
                sync):
        ext = get_extension(required=True)
        y = ext.bn_act_fwd(x_flat, res_flat, mean, invstd,
                           gamma, beta, M, C, act)
        ctx.save_for_backward(x_flat, res_flat, mean, invstd, gamma, beta)
        ctx.geom = (M, C, act, sync)
        # read once here: a graph built in deterministic mode stays
        # deterministic when .backward() runs after the mode is left
        ctx.det = is_deterministic()
        return y

    @staticmethod
    def backward(ctx, gy):
        ext = get_extension(required=True)
        x_flat, res_flat, mean, invstd, gamma, beta = ctx.saved_tensors
        M, C, act, sync = ctx.geom
        gy = gy.contiguous()
        red = ext.bn_act_bwd_reduce(x_flat, res_flat, gy, mean, invstd,
                                    gamma, beta, M, C, act, 0, ctx.det)
        # SyncBN backward: dx needs the GLOBAL (dbeta, dgamma) sums and the
        # global batch count; the returned parameter grads stay LOCAL (DDP
        # averages them afterwards, matching torch SyncBatchNorm + DDP).
        # Only the in-place all-reduce below overwrites `red`, so the local
        # grads need copies under sync alone; otherwise views do.
        dbeta, dgamma = red[:C], red[C:]
        M_norm = M
        if sync:
            dbeta, dgamma = dbeta.clone(), dgamma.clone()
            torch.distributed.all_reduce(red)
            M_norm = M * torch.distributed.get_world_size()
        dx, dres = ext.bn_act_bwd_dx(x_flat, res_flat, gy, mean, invstd,
                                     gamma, beta, red, M, C, act, M_norm)
        return (dx, dres if act == _ACT["add_relu"] else None, None, None,
                dgamma, dbeta, None, None, None, None)


def compact_enabled() -> bool:
    """MINE_BN_COMPACT=0 keeps every layer on the four-launch path (A/B in
    one build); read per call, so a test can flip it."""
    return os.environ.get("MINE_BN_COMPACT", "1") != "0"


_PLAN = {}


def _plan_says_small(ext, M: int, C: int, dtype) -> bool:
    key = (M, C, dtype)
    if key not in _PLAN:
        _PLAN[key] = bool(ext._bn.small_plan(M, C, dtype)[0])
    return _PLAN[key]


class _BNActSmallFn(torch.autograd.Function):
    """The small-layer path (bn_kernels.hip): per direction one reduction
    into a few partial rows and one consumer that finishes the sum itself.
    The forward consumer also stores mean / invstd, updates the running
    statistics and increments num_batches_tracked — `bufs`, a plain tuple,
    so autograd does not see the buffers."""

    @staticmethod
    def forward(ctx, x_flat, res_flat, gamma, beta, bufs, M, C, act, eps,
                mom):
        bn = get_extension(required=True)._bn
        ws = bn.stats_partials(x_flat, M, C)
        y, mean, invstd = bn.act_fwd_ws(x_flat, res_flat, ws, gamma, beta, M,
                                        C, act, *bufs, eps, mom)
        ctx.save_for_backward(x_flat, res_flat, mean, invstd, gamma, beta)
        ctx.geom = (M, C, act)
        return y

    @staticmethod
    def backward(ctx, gy):
        bn = get_extension(required=True)._bn
        x_flat, res_flat, mean, invstd, gamma, beta = ctx.saved_tensors
        M, C, act = ctx.geom
        gy = gy.contiguous()
        ws = bn.bwd_reduce_partials(x_flat, res_flat, gy, mean, invstd, gamma,
                                    beta, M, C, act)
        dx, dres, red = bn.act_bwd_dx_ws(x_flat, res_flat, gy, mean, invstd,
                                         gamma, beta, ws, M, C, act)
        return (dx, dres if act == _ACT["add_relu"] else None, red[C:],
                red[:C], None, None, None, None, None, None)


class _JoinStatsFn(torch.autograd.Function):
    """x = (y_base[b] + bias[b,s]) + y_dec[b,s] with the per-channel
    (sum, sumsq) of x from the same pass (bn_join_stats_vec_kernel).

    y_dec (B*S,K,H,W) and y_base (B,K,H,W) are channels_last and bias is
    (B*S,K), all bf16 or all fp16. x is bit-identical to the eager chain in
    that dtype."""

    @staticmethod
    def forward(ctx, y_dec, y_base, bias, B, S):
        ext = get_extension(required=True)
        det = is_deterministic()
        _, K, H, W = y_dec.shape
        x_flat, sums = ext.bn_join_stats(
            y_dec.permute(0, 2, 3, 1).reshape(-1),
            y_base.permute(0, 2, 3, 1).reshape(-1),
            bias.contiguous(), B, S, H * W, K, 0, det)
        ctx.geom = (B, S, H, W, K)
        ctx.det = det  # backward below sums with torch ops only
        ctx.mark_non_differentiable(sums)
        return x_flat.view(B * S, H, W, K).permute(0, 3, 1, 2), sums

    @staticmethod
    def backward(ctx, g, _gsums):
        B, S, H, W, K = ctx.geom
        g_nhwc = g.permute(0, 2, 3, 1)
        g_base = g_nhwc.reshape(B, S, H, W, K).sum(1).permute(0, 3, 1, 2)
        return g, g_base, g_nhwc.sum((1, 2)), None, None


def join_stats_usable(y_dec: torch.Tensor, y_base: torch.Tensor) -> bool:
    """True where the fused join kernel applies: bf16 or fp16 channels_last
    on the GPU with a 16-byte channel vector; everything else joins
    eagerly."""
    return (y_dec.is_cuda and y_dec.dim() == 4
            and y_dec.dtype in (torch.bfloat16, torch.float16)
            and y_base.dtype == y_dec.dtype
            and y_dec.shape[1] % 8 == 0
            and y_dec.is_contiguous(memory_format=torch.channels_last)
            and y_base.is_contiguous(memory_format=torch.channels_last))


def join_stats(y_dec, y_base, bias, B: int, S: int):
    """Fused SplitConvBlock join; returns (x, sums) with sums the (2C,)
    fp32 buffer `FusedBNAct.forward(x, sums=sums)` consumes."""
    return _JoinStatsFn.apply(y_dec, y_base, bias.to(y_dec.dtype), B, S)


def _act_eager(act: str, z: torch.Tensor) -> torch.Tensor:
    if act == "relu":
        return F.relu(z)
    if act == "lrelu":
        return F.leaky_relu(z, 0.1)
    if act == "elu":
        return F.elu(z)
    return z


class FusedBNAct(nn.BatchNorm2d):
    """BatchNorm2d with a fused activation epilogue.

    act: "none" | "relu" | "lrelu" | "elu" | "add_relu".
    For "add_relu", forward takes the residual as the second argument.
    """

    def __init__(self, num_features: int, act: str = "none", **kw):
        super().__init__(num_features, **kw)
        assert act in _ACT, act
        self.act = act
        # Cross-rank statistics sync (the reference's SyncBatchNorm role,
        # ref synthesis_task.py:106-112): when True and a process group is
        # live, the per-channel (sum, sumsq) vectors are all-reduced
        # before normalization — one 2C-float RCCL collective per BN.
        # Enabled by SynthesisTask when training.sync_batchnorm is set;
        # torch's convert_sync_batchnorm would silently DROP the fused
        # activation, so it must not be used on this module.
        self.sync = False

    def _fallback(self, x, res):
        xf = x.float()
        z = F.batch_norm(
            xf, self.running_mean, self.running_var, self.weight, self.bias,
            self.training, self.momentum, self.eps)
        if self.act == "add_relu":
            z = F.relu(z + res.float())
        else:
            z = _act_eager(self.act, z)
        return z.to(x.dtype)

    def forward(self, x: torch.Tensor, res: torch.Tensor = None,
                sums: torch.Tensor = None):
        """`sums`: optional precomputed fp32 (2C,) per-channel (sum, sumsq)
        of `x` (from `join_stats`); the training path then skips its own
        statistics launch. Ignored by the fallback and in eval mode."""
        assert (res is not None) == (self.act == "add_relu")
        use_kernel = (
            x.is_cuda and x.dim() == 4
            and x.dtype in (torch.float32, torch.bfloat16, torch.float16)
            and x.is_contiguous(memory_format=torch.channels_last)
            and (res is None or (res.dtype == x.dtype and res.is_contiguous(
                memory_format=torch.channels_last)))
            and (self.training or not torch.is_grad_enabled()))
        if not use_kernel:
            return self._fallback(x, res)

        ext = get_extension(required=True)
        B, C, H, W = x.shape
        M = B * H * W
        x_flat = x.permute(0, 2, 3, 1).reshape(-1)
        res_flat = res.permute(0, 2, 3, 1).reshape(-1) if res is not None \
            else torch.empty(0, device=x.device, dtype=x.dtype)

        do_sync = self.training and self.sync and \
            torch.distributed.is_initialized() and \
            torch.distributed.get_world_size() > 1
        if (self.training and not do_sync and sums is None
                and self.momentum is not None and compact_enabled()
                and _plan_says_small(ext, M, C, x.dtype)):
            # two launches per direction; the forward consumer does the
            # finalize, the running update and the batch count
            empty = torch.empty(0, device=x.device, dtype=torch.float32)
            track = self.track_running_stats and self.running_mean is not None
            nbt = self.num_batches_tracked
            bufs = (self.running_mean if track else empty,
                    self.running_var if track else empty,
                    nbt if nbt is not None else empty)
            y = _BNActSmallFn.apply(
                x_flat, res_flat, self.weight.float(), self.bias.float(),
                bufs, M, C, _ACT[self.act], self.eps, self.momentum)
            return y.view(B, H, W, C).permute(0, 3, 1, 2)
        if self.training:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
            mom = self.momentum if self.momentum is not None else \
                1.0 / float(self.num_batches_tracked)
            track = self.track_running_stats and self.running_mean is not None
            empty = torch.empty(0, device=x.device, dtype=torch.float32)
            if do_sync:
                if sums is None:
                    sums = ext.bn_sums(x_flat.detach(), M, C, 0,
                                       is_deterministic())
                torch.distributed.all_reduce(sums)
                Mg = M * torch.distributed.get_world_size()
                mean = sums[:C] / Mg
                var = (sums[C:] / Mg - mean * mean).clamp_min_(0.0)
                invstd = torch.rsqrt(var + self.eps)
                if track:
                    with torch.no_grad():
                        self.running_mean += mom * (mean - self.running_mean)
                        unbiased = var * Mg / max(Mg - 1, 1)
                        self.running_var += mom * (unbiased - self.running_var)
                mean = mean.contiguous()
                invstd = invstd.contiguous()
            elif sums is None:
                mean, invstd = ext.bn_stats(
                    x_flat.detach(), M, C,
                    self.running_mean if track else empty,
                    self.running_var if track else empty,
                    self.eps, mom, 0, is_deterministic())
            else:
                mean, invstd = ext.bn_finalize(
                    sums, M, C,
                    self.running_mean if track else empty,
                    self.running_var if track else empty,
                    self.eps, mom)
        else:
            mean = self.running_mean.float()
            invstd = torch.rsqrt(self.running_var.float() + self.eps)

        y = _BNActFn.apply(x_flat, res_flat, mean, invstd,
                           self.weight.float(), self.bias.float(),
                           M, C, _ACT[self.act], do_sync)
        return y.view(B, H, W, C).permute(0, 3, 1, 2)

    def extra_repr(self) -> str:  # pragma: no cover
        return super().extra_repr() + f", act={self.act}"
