"""Fused BN+activation, the fused SplitConvBlock join and the
deterministic reductions in fp16.

Oracle: the fp32 fallback math (fp32 batch norm + eager activation) on
the fp16-rounded inputs and upstream gradient, as in test_bn_stream.py.
Tolerance on y and dx: that file's bf16 tolerance 1e-2 divided by 8 for
the three extra significand bits of fp16, rtol = atol = 1.25e-3; the
fp32 parameter gradients keep its rtol 1e-4, atol 1e-3.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F16 = torch.float16
ACTS = ["none", "relu", "lrelu", "elu", "add_relu"]

# tests/test_bn_stream.py::SHAPES_BOTH (the lane-map cases of a 2-byte type)
SHAPES = [
    (3, 8, 5, 7),      # Cv=1
    (2, 16, 9, 11),    # Cv=2, the flagship's hot case
    (2, 24, 5, 7),     # Cv=3, not a power of two
    (2, 64, 3, 5),     # more rows per block than rows
    (1, 520, 3, 3),    # Cv=65, more than one channel chunk
    (1, 16, 1, 1),     # M=1
]

TOL = dict(rtol=1.25e-3, atol=1.25e-3)
PTOL = dict(rtol=1e-4, atol=1e-3)


def _cl(t):
    return t.to(DEV, F16).contiguous(memory_format=torch.channels_last)


def _oracle_act(act, z, res):
    from mine_amd.ops.bn import _act_eager
    if act == "add_relu":
        return F.relu(z + res)
    return _act_eager(act, z)


def _inputs(shape, seed=31):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    return dict(x=torch.randn(B, C, H, W, generator=g),
                r=torch.randn(B, C, H, W, generator=g),
                gy=torch.randn(B, C, H, W, generator=g),
                w=torch.rand(C, generator=g) + 0.5,
                b=torch.randn(C, generator=g) * 0.2)


def _module(C, act, d):
    from mine_amd.ops.bn import FusedBNAct
    m = FusedBNAct(C, act=act).to(DEV)
    with torch.no_grad():
        m.weight.copy_(d["w"])
        m.bias.copy_(d["b"])
    return m


# C=12 is no multiple of 8: one channel per thread (V=1)
PARITY_TRAIN = [(a, s) for s in SHAPES for a in ACTS] + \
    [(a, (2, 12, 5, 7)) for a in ("elu", "add_relu")]


@pytest.mark.parametrize(
    "act,shape", PARITY_TRAIN,
    ids=[f"{'x'.join(map(str, s))}-{a}" for a, s in PARITY_TRAIN])
def test_module_parity_train(act, shape):
    B, C, H, W = shape
    d = _inputs(shape)
    m = _module(C, act, d).train()
    x = _cl(d["x"]).requires_grad_(True)
    r = _cl(d["r"]).requires_grad_(True) if act == "add_relu" else None
    y = m(x, r) if act == "add_relu" else m(x)
    assert y.dtype == F16
    y.backward(_cl(d["gy"]))

    xr = d["x"].to(F16).float().requires_grad_(True)
    rr = d["r"].to(F16).float().requires_grad_(True)
    wr = d["w"].clone().requires_grad_(True)
    br = d["b"].clone().requires_grad_(True)
    zr = torch.batch_norm(xr, wr, br, torch.zeros(C), torch.ones(C), True,
                          0.1, 1e-5, False)
    yr = _oracle_act(act, zr, rr)
    yr.backward(d["gy"].to(F16).float())

    torch.testing.assert_close(y.float().cpu(), yr.detach(), **TOL)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, **TOL)
    if act == "add_relu":
        torch.testing.assert_close(r.grad.float().cpu(), rr.grad, **TOL)
    torch.testing.assert_close(m.weight.grad.cpu(), wr.grad, **PTOL)
    torch.testing.assert_close(m.bias.grad.cpu(), br.grad, **PTOL)


@pytest.mark.parametrize("act", ACTS)
def test_module_parity_eval(act):
    shape = (2, 16, 9, 11)
    C = shape[1]
    d = _inputs(shape, seed=33)
    g = torch.Generator().manual_seed(36)
    m = _module(C, act, d).eval()
    with torch.no_grad():
        m.running_mean.copy_(torch.randn(C, generator=g) * 0.3)
        m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        x, r = _cl(d["x"]), _cl(d["r"])
        y = m(x, r) if act == "add_relu" else m(x)
        zr = F.batch_norm(d["x"].to(F16).float(), m.running_mean.cpu(),
                          m.running_var.cpu(), d["w"], d["b"], False, 0.1,
                          1e-5)
        yr = _oracle_act(act, zr, d["r"].to(F16).float())
    assert y.dtype == F16
    torch.testing.assert_close(y.float().cpu(), yr, **TOL)


def test_bn_stats_accepts_fp16():
    """Direct extension call: refused before fp16 was an element type."""
    from mine_amd.ops.backend import get_extension
    ext = get_extension(required=True)
    M, C = 2 * 9 * 11, 16
    g = torch.Generator().manual_seed(37)
    x = torch.randn(M * C, generator=g).to(DEV, F16)
    empty = torch.empty(0, device=DEV)
    mean, invstd = ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1)
    xf = x.float().view(M, C)
    torch.testing.assert_close(mean, xf.mean(0), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(
        invstd, torch.rsqrt(xf.var(0, unbiased=False) + 1e-5), rtol=1e-4,
        atol=1e-5)


@pytest.mark.parametrize("K", [16, 24])
def test_fused_join(K):
    """join_stats in fp16 against the eager fp16 join and bn_sums, and
    FusedBNAct fed (x, sums) against FusedBNAct fed the materialised
    join."""
    from mine_amd.ops.backend import get_extension
    from mine_amd.ops.bn import FusedBNAct, join_stats, join_stats_usable

    ext = get_extension(required=True)
    B, S, H, W = 2, 3, 5, 7
    g = torch.Generator().manual_seed(34)
    y_dec = _cl(torch.randn(B * S, K, H, W, generator=g))
    y_base = _cl(torch.randn(B, K, H, W, generator=g))
    bias = torch.randn(B * S, K, generator=g).to(DEV)

    x_e = (y_base.permute(0, 2, 3, 1).unsqueeze(1)
           + bias.view(B, S, 1, 1, K).to(F16)).view(B * S, H, W, K) \
        + y_dec.permute(0, 2, 3, 1)
    assert x_e.dtype == F16
    M = B * S * H * W
    sums_e = ext.bn_sums(x_e.reshape(-1), M, K)

    assert join_stats_usable(y_dec, y_base)
    x, sums = join_stats(y_dec, y_base, bias, B, S)
    assert x.dtype == F16 and x.shape == (B * S, K, H, W)
    assert x.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(x.permute(0, 2, 3, 1), x_e)
    torch.testing.assert_close(sums, sums_e, rtol=1e-5, atol=1e-5)
    for mb in (1, 3):   # the strided row loop and its carries
        x_b, sums_b = ext.bn_join_stats(
            y_dec.permute(0, 2, 3, 1).reshape(-1),
            y_base.permute(0, 2, 3, 1).reshape(-1), bias.to(F16), B, S,
            H * W, K, mb)
        assert torch.equal(x_b.view(B * S, H, W, K), x_e)
        torch.testing.assert_close(sums_b, sums_e, rtol=1e-5, atol=1e-5)

    m1 = FusedBNAct(K, act="elu").to(DEV).train()
    m2 = FusedBNAct(K, act="elu").to(DEV).train()
    x_mat = x_e.contiguous().permute(0, 3, 1, 2)
    assert x_mat.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y1 = m1(x, sums=sums)
        y2 = m2(x_mat)
    assert y1.dtype == F16
    # same x; the statistics differ only by the fp32 summation order
    torch.testing.assert_close(y1.float(), y2.float(), **TOL)
    torch.testing.assert_close(m1.running_var, m2.running_var, rtol=1e-5,
                               atol=1e-5)


@pytest.mark.parametrize("act", ["elu", "add_relu"])
def test_deterministic_layer_is_bit_reproducible(act):
    from mine_amd.ops import deterministic
    shape = (4, 16, 96, 128)    # 384 reduction blocks without forcing
    C = shape[1]
    d = _inputs(shape, seed=45)

    def run():
        m = _module(C, act, d).train()
        x = _cl(d["x"]).requires_grad_(True)
        r = _cl(d["r"]).requires_grad_(True) if act == "add_relu" else None
        with deterministic():
            y = m(x, r) if act == "add_relu" else m(x)
            y.backward(_cl(d["gy"]))
        out = [y.detach(), x.grad, m.weight.grad, m.bias.grad,
               m.running_mean.clone(), m.running_var.clone()]
        return out + ([r.grad] if r is not None else [])

    a, b = run(), run()
    assert a[0].dtype == F16
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"output {i} differs"
