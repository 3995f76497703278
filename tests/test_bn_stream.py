"""Fused BN+activation stream kernels: lane-map cases (bf16 V=8, fp32
V=4, and V=1 where C is no multiple of that), forced small grids, eval
mode, the fused SplitConvBlock join and its decoder-level equivalence
with the eager join.

Oracle and tolerances follow tests/test_gpu_ops.py
(test_fused_bn_act_matches_torch / test_fused_bn_add_relu_matches_torch):
fp32 eager batch norm + activation on the SAME quantised inputs and
upstream gradient; rtol=atol=1e-2 (bf16) / 1e-4 (fp32) on y, x.grad and
res.grad; rtol=1e-4, atol=1e-3 on weight.grad and bias.grad.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = ["none", "relu", "lrelu", "elu", "add_relu"]

# (N,C,H,W): the smallest shapes at which each lane-map case can go wrong
SHAPES_BOTH = [
    (3, 8, 5, 7),      # bf16 Cv=1
    (2, 16, 9, 11),    # bf16 Cv=2, the flagship's hot case
    (2, 24, 5, 7),     # bf16 Cv=3, not a power of two
    (2, 64, 3, 5),     # more rows per block than rows
    (1, 520, 3, 3),    # bf16 Cv=65, more than one channel chunk
    (1, 16, 1, 1),     # M=1
]
SHAPES_F32_ONLY = [(3, 4, 5, 7), (2, 12, 5, 7)]  # fp32 Cv=1 and Cv=3
# C no multiple of 16 bytes: one channel per thread (V=1)
SHAPES_V1_BF16 = [
    (2, 12, 5, 7),     # group of 16 with four idle lanes
    (1, 70, 3, 3),     # two channel chunks, the second partial
    (1, 12, 1, 1),     # M=1
]
SHAPES_V1_F32 = [(2, 6, 5, 7)]

PARITY_CASES = [(torch.bfloat16, s) for s in SHAPES_BOTH] + \
    [(torch.float32, s) for s in SHAPES_BOTH + SHAPES_F32_ONLY] + \
    [(torch.bfloat16, s) for s in SHAPES_V1_BF16] + \
    [(torch.float32, s) for s in SHAPES_V1_F32]


def _tol(dtype):
    return dict(rtol=1e-2, atol=1e-2) if dtype == torch.bfloat16 else \
        dict(rtol=1e-4, atol=1e-4)


PTOL = dict(rtol=1e-4, atol=1e-3)


def _cl(t, dtype):
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _oracle_act(act, z, res):
    from mine_amd.ops.bn import _act_eager
    if act == "add_relu":
        return F.relu(z + res)
    return _act_eager(act, z)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize(
    "dtype,shape", PARITY_CASES,
    ids=[f"{'bf16' if d == torch.bfloat16 else 'f32'}-" +
         "x".join(map(str, s)) for d, s in PARITY_CASES])
def test_module_parity(act, dtype, shape):
    from mine_amd.ops.bn import FusedBNAct

    B, C, H, W = shape
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(B, C, H, W, generator=g)
    r0 = torch.randn(B, C, H, W, generator=g)
    gy = torch.randn(B, C, H, W, generator=g)
    w0 = torch.rand(C, generator=g) + 0.5
    b0 = torch.randn(C, generator=g) * 0.2

    m = FusedBNAct(C, act=act).to(DEV).train()
    with torch.no_grad():
        m.weight.copy_(w0)
        m.bias.copy_(b0)
    x = _cl(x0, dtype).requires_grad_(True)
    r = _cl(r0, dtype).requires_grad_(True) if act == "add_relu" else None
    y = m(x, r) if act == "add_relu" else m(x)
    assert y.dtype == dtype
    (y.float() * gy.to(DEV)).sum().backward()

    # fp32 oracle on the quantised inputs and upstream gradient, with the
    # module's own fp32 parameters. torch.batch_norm is what F.batch_norm
    # calls after its size check, which refuses the M=1 case.
    xr = x0.to(dtype).float().requires_grad_(True)
    rr = r0.to(dtype).float().requires_grad_(True)
    gyr = gy.to(dtype).float()
    wr = m.weight.detach().cpu().clone().requires_grad_(True)
    br = m.bias.detach().cpu().clone().requires_grad_(True)
    zr = torch.batch_norm(xr, wr, br, torch.zeros(C), torch.ones(C), True,
                          0.1, 1e-5, False)
    yr = _oracle_act(act, zr, rr)
    (yr * gyr).sum().backward()

    tol = _tol(dtype)
    torch.testing.assert_close(y.float().cpu(), yr.detach(), **tol)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, **tol)
    if act == "add_relu":
        torch.testing.assert_close(r.grad.float().cpu(), rr.grad, **tol)
    torch.testing.assert_close(m.weight.grad.cpu(), wr.grad, **PTOL)
    torch.testing.assert_close(m.bias.grad.cpu(), br.grad, **PTOL)


# (3,16,9,15) is added to the two shapes the lane-map table names: with
# one block a bf16 thread then owns four rows, so the unrolled body of
# the fwd kernel (three rows) runs as well as its tail. (2,12,9,11) is
# V=1 in both types: with one block a thread owns 12 or 13 rows, so the
# unrolled bodies of fwd (three rows) and dx (two) and both tails run.
@pytest.mark.parametrize("act", ["elu", "add_relu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(2, 16, 9, 11), (2, 24, 5, 7),
                                   (3, 16, 9, 15), (2, 12, 9, 11)])
def test_forced_small_grid(shape, dtype, act):
    from mine_amd.ops.backend import get_extension
    from mine_amd.ops.bn import _ACT

    ext = get_extension(required=True)
    B, C, H, W = shape
    M = B * H * W
    a = _ACT[act]
    g = torch.Generator().manual_seed(32)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = torch.randn(M * C, generator=g).to(DEV, dtype)
    res = torch.randn(M * C, generator=g).to(DEV, dtype) \
        if act == "add_relu" else torch.empty(0, device=DEV, dtype=dtype)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    empty = torch.empty(0, device=DEV)

    mean, invstd = ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1)
    sums = ext.bn_sums(x, M, C)
    y = ext.bn_act_fwd(x, res, mean, invstd, gamma, beta, M, C, a)
    red = ext.bn_act_bwd_reduce(x, res, gy, mean, invstd, gamma, beta, M, C,
                                a)
    dx, dres = ext.bn_act_bwd_dx(x, res, gy, mean, invstd, gamma, beta, red,
                                 M, C, a, M)
    # Only the fp32 summation order differs between grids. A sum that
    # cancels to near zero has no relative accuracy, so atol covers the
    # reordering error eps * sum|terms| ~ 6e-8 * (405 terms of O(1)).
    for mb in (1, 3):
        torch.testing.assert_close(ext.bn_sums(x, M, C, mb), sums,
                                   rtol=1e-5, atol=1e-5)
        mean_b, invstd_b = ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1, mb)
        torch.testing.assert_close(mean_b, mean, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(invstd_b, invstd, rtol=1e-5, atol=1e-5)
        y_b = ext.bn_act_fwd(x, res, mean, invstd, gamma, beta, M, C, a, mb)
        assert torch.equal(y_b, y)
        red_b = ext.bn_act_bwd_reduce(x, res, gy, mean, invstd, gamma, beta,
                                      M, C, a, mb)
        torch.testing.assert_close(red_b, red, rtol=1e-5, atol=1e-5)
        dx_b, dres_b = ext.bn_act_bwd_dx(x, res, gy, mean, invstd, gamma,
                                         beta, red, M, C, a, M, mb)
        assert torch.equal(dx_b, dx)
        assert torch.equal(dres_b, dres)


def test_eval_mode_bf16():
    from mine_amd.ops.bn import FusedBNAct

    g = torch.Generator().manual_seed(33)
    C = 16
    m = FusedBNAct(C, act="relu").to(DEV).eval()
    with torch.no_grad():
        m.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
        m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        m.weight.copy_(torch.rand(C, generator=g) + 0.5)
        m.bias.copy_(torch.randn(C, generator=g) * 0.2)
        x0 = torch.randn(2, C, 9, 11, generator=g)
        y = m(_cl(x0, torch.bfloat16))
        yr = F.relu(F.batch_norm(
            x0.to(torch.bfloat16).float(), m.running_mean.cpu(),
            m.running_var.cpu(), m.weight.cpu(), m.bias.cpu(), False, 0.1,
            1e-5))
    assert y.dtype == torch.bfloat16
    torch.testing.assert_close(y.float().cpu(), yr, **_tol(torch.bfloat16))


@pytest.mark.parametrize("K", [16, 24])
def test_fused_join(K):
    from mine_amd.ops.backend import get_extension
    from mine_amd.ops.bn import join_stats, join_stats_usable

    B, S, H, W = 2, 3, 5, 7
    bf16 = torch.bfloat16
    g = torch.Generator().manual_seed(34)
    yd0 = torch.randn(B * S, K, H, W, generator=g)
    yb0 = torch.randn(B, K, H, W, generator=g)
    bp0 = torch.randn(B * S, K, generator=g)
    gw = torch.randn(B * S, H, W, K, generator=g).to(DEV)

    def leaves():
        return (_cl(yd0, bf16).requires_grad_(True),
                _cl(yb0, bf16).requires_grad_(True),
                bp0.to(DEV).requires_grad_(True))

    # eager join, as SplitConvBlock writes it
    y_dec_e, y_base_e, bias_e = leaves()
    x_e = (y_base_e.permute(0, 2, 3, 1).unsqueeze(1)
           + bias_e.view(B, S, 1, 1, K).to(bf16)).view(B * S, H, W, K) \
        + y_dec_e.permute(0, 2, 3, 1)
    (x_e.float() * gw).sum().backward()

    y_dec, y_base, bias = leaves()
    assert join_stats_usable(y_dec, y_base)
    x, sums = join_stats(y_dec, y_base, bias, B, S)
    assert x.shape == (B * S, K, H, W) and x.dtype == bf16
    assert x.is_contiguous(memory_format=torch.channels_last)
    x_nhwc = x.permute(0, 2, 3, 1)
    assert torch.equal(x_nhwc, x_e)
    xf = x_nhwc.detach().float().reshape(-1, K)
    ref = torch.cat((xf.sum(0), xf.square().sum(0)))
    torch.testing.assert_close(sums, ref, rtol=1e-5, atol=1e-5)
    (x_nhwc.float() * gw).sum().backward()
    tol = _tol(bf16)
    torch.testing.assert_close(y_dec.grad, y_dec_e.grad, **tol)
    torch.testing.assert_close(y_base.grad, y_base_e.grad, **tol)
    torch.testing.assert_close(bias.grad, bias_e.grad, **tol)

    # the strided row loop and its (p, s, b) carries on a forced small grid
    ext = get_extension(required=True)
    flat = [y_dec.detach().permute(0, 2, 3, 1).reshape(-1),
            y_base.detach().permute(0, 2, 3, 1).reshape(-1),
            bias.detach().to(bf16)]
    for mb in (1, 3):
        x_b, sums_b = ext.bn_join_stats(*flat, B, S, H * W, K, mb)
        assert torch.equal(x_b.view(B * S, H, W, K), x_e)
        torch.testing.assert_close(sums_b, ref, rtol=1e-5, atol=1e-5)


def test_decoder_fused_join_matches_eager():
    from mine_amd.models import MPIDecoder
    from mine_amd.models.decoder import SplitConvBlock

    torch.manual_seed(35)
    B, S, H, W = 1, 2, 128, 128
    bf16 = torch.bfloat16
    num_ch_enc = [64, 256, 512, 1024, 2048]
    dec = MPIDecoder(num_ch_enc).to(DEV).train()
    feats0 = [torch.randn(B, c, H >> (i + 1), W >> (i + 1))
              for i, c in enumerate(num_ch_enc)]
    disparity = torch.tensor([[0.8, 0.3]], device=DEV)
    wts = {s: torch.randn(B, S, 4, H >> s, W >> s, device=DEV)
           for s in range(4)}
    joins = [m for m in dec.modules() if isinstance(m, SplitConvBlock)]
    assert sum(1 for m in joins if m.dec_ch) == 4

    def run(fused):
        for m in joins:
            m.fused_join = fused
        dec.zero_grad(set_to_none=True)
        feats = [_cl(f, bf16) for f in feats0]
        with torch.autocast("cuda", dtype=bf16):
            out = dec(feats, disparity)
        loss = sum((out[("disp", s)].float() * wts[s]).mean()
                   for s in range(4))
        loss.backward()
        return ({s: out[("disp", s)].detach().float() for s in range(4)},
                {n: p.grad.detach().float().clone()
                 for n, p in dec.named_parameters() if p.grad is not None})

    out_f, grad_f = run(True)
    out_e, grad_e = run(False)
    tol = _tol(bf16)
    for s in range(4):
        torch.testing.assert_close(out_f[s], out_e[s], **tol)
    assert grad_f.keys() == grad_e.keys() and grad_f
    for n in grad_e:
        torch.testing.assert_close(grad_f[n], grad_e[n], **tol, msg=lambda m:
                                   f"{n}: {m}")
