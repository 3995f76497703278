"""Deterministic mode past the network's last layer: the order-fixed warp
backward (mode 2: emit + `tgt_collect`), the order-fixed SSIM and
smoothness reductions, the atomic-free sparse-point gather backward, and
one whole train step repeated from the same state.

Exactness tests use dyadic geometry (u = x/4 + c, v = y/2 + c', so every
bilinear weight is a multiple of 1/16) and small-integer payloads: every
fp32 summation order is exact and the only way to be wrong is to miss,
double or misassign a pixel. Order tests put 2^24 next to 1 with
alternating signs, so that an fp32 sum depends on the order of its
addends, and demand bit-identical results call after call.

Parity bounds are those of the existing tests of the same kernels:
tests/test_render_paths_gpu.py::_check_tgt for the warp backward, and
max(16 * dev32, 1e-5 * max|ref|) of tests/test_ssim_paths_gpu.py and
tests/test_smooth_paths_gpu.py for the losses (dev32 = deviation of the
fp32 eager CPU path from the fp64 one on the same inputs).

The scenes' properties (clamped shares, corner texels, duplicate points)
are asserted on the CPU in tests/test_collect_sim.py.
"""
import copy
import functools

import pytest
import torch

import test_collect_sim as sim
import test_render_paths_gpu as rp
from mine_amd.utils.geometry import inverse_3x3

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPEATS = 5


def _ext():
    from mine_amd.ops.backend import get_extension
    return get_extension(required=True)


@pytest.fixture
def restore_mode():
    from mine_amd.ops import backend, conv
    prev = (backend._DETERMINISTIC, conv._FORCE_IGEMM,
            torch.backends.cudnn.deterministic)
    yield
    backend._DETERMINISTIC = prev[0]
    conv.set_force_igemm(prev[1])
    torch.backends.cudnn.deterministic = prev[2]


def _spy(monkeypatch, name, log):
    ext = _ext()
    real = getattr(ext, name)

    def wrapper(*args, **kw):
        log.append((name, args, kw))
        return real(*args, **kw)

    monkeypatch.setattr(ext, name, wrapper)


# ---------------------------------------------------------------------------
# tgt_collect on a given payload
# ---------------------------------------------------------------------------

COLLECT_CASES = {
    "2x3x37x45": (2, 3, 37, 45, sim.DYADIC_37x45),
    "2x1x9x11": (2, 1, 9, 11, sim.DYADIC_9x11),
}


@functools.lru_cache(maxsize=None)
def _collect_case(name):
    B, S, H, W, offsets = COLLECT_CASES[name]
    assert (H * W) % 256 != 0 and len(offsets) == B * S
    hinv = sim.dyadic_hinv(offsets).reshape(B, S, 3, 3)
    hfwd = inverse_3x3(hinv.reshape(B * S, 3, 3)).reshape(B, S, 3, 3)
    # the fp32 inverse of a dyadic map is exact
    eye = torch.matmul(hinv.double(), hfwd.double())
    assert torch.equal(eye, torch.eye(3, dtype=torch.float64).expand_as(eye))
    g = torch.Generator().manual_seed(70 + H)
    ints = torch.randint(-8, 9, (B, S, H, W, 4), generator=g).float()
    # 2^24 next to 1, signs alternating along x
    big = torch.rand(B, S, H, W, 4, generator=g) < 0.5
    sign = 1.0 - 2.0 * (torch.arange(W) % 2).float().view(1, 1, 1, W, 1)
    mixed = torch.where(big, torch.tensor(2.0 ** 24), torch.tensor(1.0)) * sign
    return dict(hinv=hinv, hfwd=hfwd, ints=ints, mixed=mixed.contiguous(),
                ref=sim.scatter_reference(ints, hinv))


def _collect(payload, hinv, hfwd):
    return _ext().tgt_collect(payload.to(DEV), hinv.to(DEV).contiguous(),
                              hfwd.to(DEV).contiguous())


@pytest.mark.parametrize("name", sorted(COLLECT_CASES))
def test_tgt_collect_exact_on_dyadic_integers(name):
    c = _collect_case(name)
    assert c["ref"].abs().max() < 2 ** 20   # exact in fp32 in any order
    got = _collect(c["ints"], c["hinv"], c["hfwd"])
    assert got.dtype == torch.float32 and got.shape == c["ints"].shape
    # every unit of payload arrives somewhere exactly once
    assert torch.equal(got.double().sum((2, 3)).cpu(),
                       c["ints"].double().sum((2, 3)))
    bad = (got.double().cpu() != c["ref"]).sum().item()
    assert torch.equal(got.double().cpu(), c["ref"]), f"{bad} entries differ"


@pytest.mark.parametrize("name", sorted(COLLECT_CASES))
def test_tgt_collect_order_is_fixed(name):
    c = _collect_case(name)
    first = _collect(c["mixed"], c["hinv"], c["hfwd"])
    assert bool(torch.isfinite(first).all())
    for i in range(REPEATS - 1):
        again = _collect(c["mixed"], c["hinv"], c["hfwd"])
        assert torch.equal(again, first), f"call {i + 2} differs"
    alone = _collect(c["mixed"][:1], c["hinv"][:1], c["hfwd"][:1])
    assert torch.equal(alone[0], first[0])
    # the payload really is order-sensitive: the fp64 sum is not what
    # fp32 gives in every order
    ref = sim.scatter_reference(c["mixed"], c["hinv"])
    assert not torch.equal(ref.float().double(), ref)


# ---------------------------------------------------------------------------
# mode 2 end to end
# ---------------------------------------------------------------------------

MODE2_CASES = [(n, bg, False) for n in ("odd", "cull", "exit", "few1", "few2")
               for bg in (False, True)] + \
              [("odd", False, True), ("odd", True, True)]


@pytest.mark.parametrize("name,bg_inf,alpha", MODE2_CASES)
def test_mode2_matches_fp64_oracle_and_repeats(name, bg_inf, alpha,
                                               monkeypatch, restore_mode):
    from mine_amd.ops import deterministic
    log = []
    _spy(monkeypatch, "tgt_composite_bwd", log)
    with deterministic():
        # the bounds, exclusions and r factor of _check_tgt; the mode
        # argument it patches is overridden by deterministic mode
        rp._check_tgt(name, bg_inf, alpha, 1, monkeypatch)
        first = rp._run_tgt(name, DEV, torch.float32, bg_inf, alpha)
        for i in range(REPEATS - 1):
            again = rp._run_tgt(name, DEV, torch.float32, bg_inf, alpha)
            for k in ("grad_rgb", "grad_sigma"):
                assert torch.equal(again[k], first[k]), \
                    f"{k}: backward {i + 2} differs"
    assert len(log) == REPEATS + 1
    assert all(args[10] == 2 for _, args, _ in log), \
        [args[10] for _, args, _ in log]


def test_mode2_graph_keeps_its_mode_after_the_block(monkeypatch,
                                                    restore_mode):
    """The mode is read in forward: a graph built inside the block runs
    mode 2 when .backward() comes after it, and the other way round."""
    from mine_amd.ops import deterministic
    from mine_amd.ops.renderer import pack_mpi, render_tgt_view
    log = []
    _spy(monkeypatch, "tgt_composite_bwd", log)
    sc = rp._scene("few2")
    to = lambda t: t.detach().clone().to(DEV)

    def forward():
        r = to(sc["rgb"]).requires_grad_(True)
        s = to(sc["sigma"]).requires_grad_(True)
        out = render_tgt_view(pack_mpi(r, s), to(sc["disparity"]),
                              to(sc["G"]), to(sc["K_inv"]), to(sc["K"]))
        return out[0].sum()

    with deterministic():
        inside = forward()
    inside.backward()
    with deterministic(False):
        outside = forward()
    with deterministic():
        outside.backward()
    assert [args[10] for _, args, _ in log] == [2, 1]


# ---------------------------------------------------------------------------
# SSIM and smoothness in the mode
# ---------------------------------------------------------------------------

def _bound(dev32, ref):
    return max(16.0 * dev32, 1e-5 * ref.abs().max().item())


SSIM_SHAPES = [(2, 3, 37, 45), (1, 3, 7, 9)]
SSIM_UPSTREAM = -3.0


@functools.lru_cache(maxsize=None)
def _ssim_case(shape):
    """Pair with per-channel magnitudes 1, 0.1, 0.01, and its fp64 value
    and gradient with the fp32 eager deviations."""
    from mine_amd.ops.ssim import ssim
    g = torch.Generator().manual_seed(80 + shape[2])
    mag = torch.tensor([1.0, 0.1, 0.01]).view(1, 3, 1, 1)
    a = torch.rand(*shape, generator=g) * mag
    b = torch.rand(*shape, generator=g) * mag

    def eager(dtype):
        x = a.clone().to(dtype).requires_grad_(True)
        val = ssim(x, b.to(dtype), force_torch=True)
        (val * SSIM_UPSTREAM).backward()
        return val.detach().double(), x.grad.double()

    v64, g64 = eager(torch.float64)
    v32, g32 = eager(torch.float32)
    return dict(a=a, b=b, val=v64, grad=g64,
                dev_val=(v32 - v64).abs().item(),
                dev_grad=(g32 - g64).abs().max().item())


@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_deterministic(shape, monkeypatch, restore_mode):
    from mine_amd.ops import deterministic
    from mine_amd.ops.ssim import ssim
    c = _ssim_case(shape)
    log = []
    _spy(monkeypatch, "ssim_fwd", log)

    def run():
        x = c["a"].to(DEV).requires_grad_(True)
        with deterministic():
            val = ssim(x, c["b"].to(DEV))
        (val * SSIM_UPSTREAM).backward()
        return val.detach(), x.grad

    val, grad = run()
    for i in range(REPEATS - 1):
        v2, g2 = run()
        assert torch.equal(v2, val), f"value: call {i + 2} differs"
        assert torch.equal(g2, grad), f"gradient: call {i + 2} differs"
    assert len(log) == REPEATS and all(args[2] is True for _, args, _ in log)

    b_val = _bound(c["dev_val"], c["val"])
    b_grad = _bound(c["dev_grad"], c["grad"])
    e_val = (val.double().cpu() - c["val"]).abs().item()
    e_grad = (grad.double().cpu() - c["grad"]).abs().max().item()
    print(f"ssim det {shape}: value err/bound = {e_val / b_val:.3g} (err "
          f"{e_val:.2e}, bound {b_val:.2e}); grad err/bound = "
          f"{e_grad / b_grad:.3g} (err {e_grad:.2e}, bound {b_grad:.2e})")
    assert e_val <= b_val
    assert e_grad <= b_grad
    # the two modes differ by summation order alone
    dflt = ssim(c["a"].to(DEV), c["b"].to(DEV))
    assert (dflt - val).abs().item() <= 2.0 * b_val


EAV2_SHAPES = [(2, 37, 45), (2, 520, 520)]   # (B, H, W)
EAV2_UPSTREAM = 3.0


@functools.lru_cache(maxsize=None)
def _eav2_case(shape):
    """Disparities with per-image means a factor 100 apart (so the T_b
    term of the backward differs per image and shows in the gradient)."""
    from mine_amd.ops.losses import edge_aware_loss_v2
    B, H, W = shape
    g = torch.Generator().manual_seed(90 + H)
    img = torch.rand(B, 3, H, W, generator=g)
    d = (torch.rand(B, 1, H, W, generator=g) * 2 + 0.1) * \
        torch.tensor([0.1, 10.0]).view(B, 1, 1, 1)

    def eager(dtype):
        x = d.clone().to(dtype).requires_grad_(True)
        loss = edge_aware_loss_v2(img.to(dtype), x)
        (loss * EAV2_UPSTREAM).backward()
        return loss.detach().double(), x.grad.double()

    l64, g64 = eager(torch.float64)
    l32, g32 = eager(torch.float32)
    return dict(img=img, d=d.contiguous(), loss=l64, grad=g64,
                dev_loss=(l32 - l64).abs().item(),
                dev_grad=(g32 - g64).abs().max().item())


@pytest.mark.parametrize("shape", EAV2_SHAPES)
def test_eav2_deterministic(shape, monkeypatch, restore_mode):
    from mine_amd.ops import deterministic
    from mine_amd.ops.losses import edge_aware_loss_v2
    B, H, W = shape
    if H == 520:   # reaches the capped 1024-block grid of loss_kernels.hip
        assert (H * W + 255) // 256 > 1024
    c = _eav2_case(shape)
    log = []
    _spy(monkeypatch, "eav2_fwd", log)
    _spy(monkeypatch, "eav2_bwd", log)
    img = c["img"].to(DEV)

    def run():
        x = c["d"].to(DEV).requires_grad_(True)
        with deterministic():
            loss = edge_aware_loss_v2(img, x)
        assert "EdgeAwareV2" in type(loss.grad_fn).__name__
        (loss * EAV2_UPSTREAM).backward()   # after the block: mode is kept
        return loss.detach(), x.grad

    loss, grad = run()
    for i in range(REPEATS - 1):
        l2, g2 = run()
        assert torch.equal(l2, loss), f"loss: call {i + 2} differs"
        assert torch.equal(g2, grad), f"gradient: call {i + 2} differs"
    assert [n for n, _, _ in log] == ["eav2_fwd", "eav2_bwd"] * REPEATS
    assert all(args[-1] is True for _, args, _ in log)

    b_l = _bound(c["dev_loss"], c["loss"])
    b_g = _bound(c["dev_grad"], c["grad"])
    e_l = (loss.double().cpu() - c["loss"]).abs().item()
    e_g = (grad.double().cpu() - c["grad"]).abs().max().item()
    print(f"eav2 det {shape}: loss err/bound = {e_l / b_l:.3g} (err "
          f"{e_l:.2e}, bound {b_l:.2e}); grad err/bound = {e_g / b_g:.3g} "
          f"(err {e_g:.2e}, bound {b_g:.2e})")
    assert e_l <= b_l
    assert e_g <= b_g    # T_b enters every entry of the gradient


# ---------------------------------------------------------------------------
# sparse-point gather
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
def test_sparse_gather_backward_exact_and_repeatable(C, monkeypatch,
                                                     restore_mode):
    from mine_amd.ops import deterministic, gather_pixel_by_pxpy, torch_ref
    B, H, W, N = 2, 8, 12, 128
    pxpy = sim.sparse_points(B=B, H=H, W=W, N=N)
    idx = sim.flat_index(pxpy, H, W)
    g = torch.Generator().manual_seed(33)
    img = torch.rand(B, C, H, W, generator=g)
    up_int = torch.randint(-8, 9, (B, C, N), generator=g).float()
    big = torch.rand(B, C, N, generator=g) < 0.5
    sign = 1.0 - 2.0 * (torch.arange(N) % 2).float()
    up_mixed = torch.where(big, torch.tensor(2.0 ** 24),
                           torch.tensor(1.0)) * sign
    log = []
    _spy(monkeypatch, "gather_pxpy_bwd", log)

    def run(up):
        x = img.to(DEV).requires_grad_(True)
        with deterministic():
            out = gather_pixel_by_pxpy(x, pxpy.to(DEV))
        out.backward(up.to(DEV))
        return out.detach(), x.grad

    out, grad = run(up_int)
    assert torch.equal(out.cpu(), torch_ref.gather_pixel_by_pxpy(img, pxpy))
    ref = torch.zeros(B, C, H * W, dtype=torch.float64)
    ref.scatter_add_(2, idx.unsqueeze(1).expand(B, C, N), up_int.double())
    assert torch.equal(grad.double().cpu().reshape(B, C, H * W), ref)

    first = run(up_mixed)[1]
    for i in range(REPEATS - 1):
        assert torch.equal(run(up_mixed)[1], first), f"call {i + 2} differs"
    assert len(log) == REPEATS + 1


# ---------------------------------------------------------------------------
# default mode untouched
# ---------------------------------------------------------------------------

def test_default_mode_runs_the_default_kernels(monkeypatch, restore_mode):
    from mine_amd.ops import (deterministic, edge_aware_loss_v2,
                              gather_pixel_by_pxpy, ssim)
    from mine_amd.ops import renderer
    monkeypatch.setattr(renderer, "_TGT_BWD_MODE", None)
    monkeypatch.delenv("MINE_TGT_BWD", raising=False)
    log = []
    for name in ("tgt_composite_bwd", "tgt_collect", "ssim_fwd", "eav2_fwd",
                 "eav2_bwd", "gather_pxpy_bwd"):
        _spy(monkeypatch, name, log)
    with deterministic(False):
        rp._run_tgt("few2", DEV, torch.float32, False, False)
        c = _ssim_case(SSIM_SHAPES[1])
        x = c["a"].to(DEV).requires_grad_(True)
        ssim(x, c["b"].to(DEV)).backward()
        e = _eav2_case(EAV2_SHAPES[0])
        d = e["d"].to(DEV).requires_grad_(True)
        edge_aware_loss_v2(e["img"].to(DEV), d).backward()
        img = torch.rand(2, 1, 8, 12, device=DEV, requires_grad=True)
        out = gather_pixel_by_pxpy(img, sim.sparse_points().to(DEV))
        assert "Gather" in type(out.grad_fn).__name__ and \
            "Pxpy" not in type(out.grad_fn).__name__   # torch.gather itself
        out.sum().backward()
    calls = {n: (a, k) for n, a, k in log}
    assert [n for n, _, _ in log] == ["tgt_composite_bwd", "ssim_fwd",
                                      "eav2_fwd", "eav2_bwd"]
    assert calls["tgt_composite_bwd"][0][10] == 1
    assert calls["ssim_fwd"][0][2] is False
    assert calls["eav2_fwd"][0][-1] is False
    assert calls["eav2_bwd"][0][-1] is False
    # and the bindings' defaults are the default mode
    ext = _ext()
    a, b = c["a"].to(DEV), c["b"].to(DEV)
    v_default, = ext.ssim_fwd(a, b)
    v_det, = ext.ssim_fwd(a, b, det=True)
    assert (v_default - v_det).abs().item() <= 1e-6


# ---------------------------------------------------------------------------
# one whole train step
# ---------------------------------------------------------------------------

def test_whole_step_bit_reproducible(restore_mode):
    """One train step (all four scales, v1 smoothness on, 128 sparse
    points, a yawed target camera that clamps over 40 % of the pixels)
    run twice from the same seeded state in deterministic mode: every
    loss term, every parameter gradient and every updated parameter and
    buffer is bit-identical."""
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import is_deterministic

    cfg = sim.step_config()
    items = sim.step_items()
    torch.manual_seed(61)
    task = SynthesisTask(cfg, device=DEV)
    assert is_deterministic()
    assert cfg["loss.smoothness_lambda_v1"] != 0.0 and task.use_multi_scale
    nets = [task.backbone, task.decoder]
    state = [{k: v.clone() for k, v in n.state_dict().items()} for n in nets]
    opt_state = copy.deepcopy(task.optimizer.state_dict())

    def run():
        for n, sd in zip(nets, state):
            n.load_state_dict(sd)
        task.optimizer.load_state_dict(copy.deepcopy(opt_state))
        task.global_step = 0
        torch.manual_seed(62)        # the stratified disparity samples
        loss_dict = task.train_step(items)
        losses = {k: v.detach().clone() for k, v in loss_dict.items()}
        grads = {f"{i}.{k}": p.grad.detach().clone()
                 for i, n in enumerate(nets)
                 for k, p in n.named_parameters() if p.grad is not None}
        after = {f"{i}.{k}": v.detach().clone() for i, n in enumerate(nets)
                 for k, v in n.state_dict().items()}
        return losses, grads, after

    l1, g1, p1 = run()
    l2, g2, p2 = run()
    assert bool(torch.isfinite(l1["loss"]))
    for k in ("loss_smooth_tgt", "loss_disp_pt3dsrc", "loss_disp_pt3dtgt",
              "loss_ssim_tgt", "loss_smooth_tgt_v2"):
        assert l1[k].item() != 0.0, f"{k} is not trained in this config"
    bad = [k for k in l1 if not torch.equal(l1[k], l2[k])]
    print("loss terms that differ:", {k: (l1[k].item(), l2[k].item())
                                      for k in bad})
    assert not bad
    assert g1 and g1.keys() == g2.keys()
    bad = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    worst = max(((g1[k] - g2[k]).abs().max().item() for k in bad),
                default=0.0)
    print(f"{len(bad)} of {len(g1)} gradients differ, max |diff| = {worst:.3e}"
          f": {bad[:8]}")
    assert not bad
    bad = [k for k in p1 if not torch.equal(p1[k], p2[k])]
    assert not bad, f"{len(bad)} of {len(p1)} updated tensors differ: {bad[:8]}"
    # the step moved the parameters
    moved = [k for k in p1 if k.endswith("weight") and
             not torch.equal(p1[k], state[int(k[0])][k[2:]])]
    assert moved
