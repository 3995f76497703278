"""HIP extension loader.

The extension `_mine_hip` is built IN-TREE (mine_amd/ops/_mine_hip*.so)
by `python setup.py build_ext --inplace` / `__graft_entry__.build()` for
gfx950 only. There is no JIT fallback and no CPU shim inside the
extension: on a CUDA (ROCm) device the fused kernels are REQUIRED — if
the extension is missing, ops fail loudly rather than silently falling
back to eager PyTorch.
"""
from __future__ import annotations

import contextlib
import importlib
from typing import Optional

_EXT = None
_TRIED = False
_ERR: Optional[BaseException] = None


def get_extension(required: bool = False):
    global _EXT, _TRIED, _ERR
    if not _TRIED:
        _TRIED = True
        try:
            _EXT = importlib.import_module("mine_amd.ops._mine_hip")
        except Exception as e:  # noqa: BLE001
            _EXT = None
            _ERR = e
    if _EXT is None and required:
        raise RuntimeError(
            "mine_amd HIP extension (_mine_hip) is not built. Build it with "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error: {_ERR!r}")
    return _EXT


def has_extension() -> bool:
    return get_extension(required=False) is not None


# ---------------------------------------------------------------------------
# Deterministic mode (off by default).
#
# When on, every reduction inside the network — the BN statistics and
# backward reductions, `bias_grad`, the igemm split-K forward / data
# gradient and the igemm weight gradient — combines its partial sums in
# an order that depends only on the shapes (per-block / per-slice
# partials in a workspace, summed by a finishing kernel) instead of with
# fp32 atomics. Past the network, the novel-view warp backward runs its
# order-fixed emit + collect form (mode 2), the SSIM / smoothness
# scalars and the smoothness backward's per-image dot are summed the
# same workspace way, the sparse-point gather gets an atomic-free
# backward and the v1 smoothness Sobel is built from slices. One train
# step on one GPU is then bit-reproducible: losses, gradients, updated
# parameters. Not covered: the RCCL all-reduce order (docs/NEXT.md
# section 7).
#
# The initial value is read lazily from MINE_DETERMINISTIC=1, the same
# convention as MINE_TGT_BWD / MINE_CONV_BWD. The autograd functions read
# the mode once in forward and keep it for their backward.
# ---------------------------------------------------------------------------

_DETERMINISTIC: Optional[bool] = None  # lazy: MINE_DETERMINISTIC


def is_deterministic() -> bool:
    global _DETERMINISTIC
    if _DETERMINISTIC is None:
        import os
        _DETERMINISTIC = os.environ.get("MINE_DETERMINISTIC", "0") == "1"
        if _DETERMINISTIC:
            # as training.deterministic does: the convs that stay on the
            # library (the 7x7 stem's weight gradient) must not pick an
            # atomic kernel either
            import torch
            torch.backends.cudnn.deterministic = True
    return _DETERMINISTIC


def set_deterministic(enabled: bool) -> None:
    global _DETERMINISTIC
    _DETERMINISTIC = bool(enabled)


@contextlib.contextmanager
def deterministic(enabled: bool = True):
    """Run the body in (or, with enabled=False, out of) deterministic
    mode; the previous value is restored on exit."""
    prev = is_deterministic()
    set_deterministic(enabled)
    try:
        yield
    finally:
        set_deterministic(prev)
