"""Deterministic mode on the GPU: the order-fixed BN reductions, igemm
split-K forward / data gradient and igemm weight gradient.

Exactness tests use small-integer data, for which every fp32 summation
order is exact (all partials and totals stay below 2^24): the only way to
be wrong is to drop or double-count a partial. Repeatability tests use
standard-normal data and demand bit-identical results call after call.
Parity tests reuse the oracle and tolerances of tests/test_bn_stream.py.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF16, F32 = torch.bfloat16, torch.float32
ACTS = ["none", "relu", "lrelu", "elu", "add_relu"]

# tests/test_bn_stream.py::SHAPES_BOTH / SHAPES_F32_ONLY (lane-map cases)
SHAPES_BOTH = [
    (3, 8, 5, 7),
    (2, 16, 9, 11),
    (2, 24, 5, 7),
    (2, 64, 3, 5),
    (1, 520, 3, 3),
    (1, 16, 1, 1),
]
SHAPES_F32_ONLY = [(3, 4, 5, 7), (2, 12, 5, 7)]
GENERIC_BF16 = (2, 12, 5, 7)     # C % 8 != 0: one channel per thread (V=1)
BIG_BF16 = (4, 16, 96, 128)      # 384 blocks without forcing

SUM_CASES = [(BF16, s) for s in SHAPES_BOTH] + \
    [(F32, s) for s in SHAPES_BOTH + SHAPES_F32_ONLY] + \
    [(BF16, GENERIC_BF16), (BF16, BIG_BF16)] + \
    [(F32, (2, 6, 5, 7)), (BF16, (1, 70, 3, 3))]    # V=1 as well
PARITY_CASES = [(BF16, s) for s in SHAPES_BOTH] + \
    [(F32, s) for s in SHAPES_BOTH] + [(BF16, GENERIC_BF16)]


def _id(case):
    d, s = case
    return ("bf16-" if d == BF16 else "f32-") + "x".join(map(str, s))


# test_bn_stream.py::_tol / PTOL
def _tol(dtype):
    return dict(rtol=1e-2, atol=1e-2) if dtype == BF16 else \
        dict(rtol=1e-4, atol=1e-4)


PTOL = dict(rtol=1e-4, atol=1e-3)


def _ext():
    from mine_amd.ops.backend import get_extension
    return get_extension(required=True)


def _cl(t, dtype):
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g)


@pytest.fixture
def restore_mode():
    from mine_amd.ops import backend, conv
    prev = (backend._DETERMINISTIC, conv._FORCE_IGEMM,
            torch.backends.cudnn.deterministic)
    yield
    backend._DETERMINISTIC = prev[0]
    conv.set_force_igemm(prev[1])
    torch.backends.cudnn.deterministic = prev[2]


# ---------------------------------------------------------------------------
# BN sums exact on integer data
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", SUM_CASES, ids=_id)
def test_bn_sums_exact_on_integers(case):
    dtype, (B, C, H, W) = case
    ext = _ext()
    M = B * H * W
    assert M < 1 << 19  # |sum| <= 4M, sumsq <= 16M < 2^24
    xi = _ints((M, C), -4, 4, 41)
    exact = torch.cat((xi.sum(0), (xi * xi).sum(0))).float()
    x = xi.reshape(-1).to(DEV, dtype)
    for mb in (0, 1, 3):
        sums = ext.bn_sums(x, M, C, mb, deterministic=True)
        assert torch.equal(sums.cpu(), exact), f"max_blocks={mb}"


@pytest.mark.parametrize("case", SUM_CASES, ids=_id)
def test_bn_bwd_reduce_dbeta_exact_on_integers(case):
    dtype, (B, C, H, W) = case
    ext = _ext()
    M = B * H * W
    gi = _ints((M, C), -4, 4, 42)
    exact = gi.sum(0).float()
    g = torch.Generator().manual_seed(43)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = gi.reshape(-1).to(DEV, dtype)
    res = torch.empty(0, device=DEV, dtype=dtype)
    mean = torch.randn(C, generator=g).to(DEV)
    invstd = (torch.rand(C, generator=g) + 0.5).to(DEV)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    for mb in (0, 1, 3):
        red = ext.bn_act_bwd_reduce(x, res, gy, mean, invstd, gamma, beta, M,
                                    C, 0, mb, deterministic=True)
        assert red.shape == (2 * C,)
        assert torch.equal(red[:C].cpu(), exact), f"max_blocks={mb}"


@pytest.mark.parametrize("K", [16, 4])
def test_bias_grad_exact_on_integers(K, restore_mode):
    from mine_amd.ops import deterministic
    from mine_amd.ops.conv import bias_grad
    B, H, W = 2, 9, 70
    gi = _ints((B, K, H, W), -4, 4, 44)
    exact = gi.sum((0, 2, 3)).float()
    gy = _cl(gi, BF16)
    with deterministic():
        gb = bias_grad(gy)
    assert gb.dtype == F32 and torch.equal(gb.cpu(), exact)


# ---------------------------------------------------------------------------
# repeatability
# ---------------------------------------------------------------------------

def _all_equal(a, b):
    a = a if isinstance(a, (list, tuple)) else [a]
    b = b if isinstance(b, (list, tuple)) else [b]
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("dtype,shape,mb", [
    (BF16, BIG_BF16, 0), (BF16, GENERIC_BF16, 3), (F32, GENERIC_BF16, 3)],
    ids=["bf16-4x16x96x128", "bf16-2x12x5x7-mb3", "f32-2x12x5x7-mb3"])
def test_bn_repeatable(dtype, shape, mb):
    from mine_amd.ops.bn import _ACT
    ext = _ext()
    B, C, H, W = shape
    M = B * H * W
    g = torch.Generator().manual_seed(45)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = torch.randn(M * C, generator=g).to(DEV, dtype)
    res = torch.randn(M * C, generator=g).to(DEV, dtype)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    empty = torch.empty(0, device=DEV)
    none = torch.empty(0, device=DEV, dtype=dtype)

    calls = {
        "bn_sums": lambda: ext.bn_sums(x, M, C, mb, deterministic=True),
        "bn_stats": lambda: ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1, mb,
                                         deterministic=True),
    }
    mean, invstd = calls["bn_stats"]()
    for act in ACTS:
        a = _ACT[act]
        r = res if act == "add_relu" else none
        calls["bwd_reduce-" + act] = (
            lambda a=a, r=r: ext.bn_act_bwd_reduce(
                x, r, gy, mean, invstd, gamma, beta, M, C, a, mb,
                deterministic=True))
    if dtype == BF16 and C % 8 == 0:
        # the fused join is bf16 with a 16-byte channel vector only
        Bj, Sj, HW = 2, B // 2, H * W
        y_base = torch.randn(Bj * HW * C, generator=g).to(DEV, dtype)
        bias = torch.randn(Bj * Sj * C, generator=g).to(DEV, dtype)
        calls["bn_join_stats"] = lambda: ext.bn_join_stats(
            x, y_base, bias, Bj, Sj, HW, C, mb, deterministic=True)

    for name, fn in calls.items():
        first = fn()
        for i in range(9):
            assert _all_equal(fn(), first), f"{name}: call {i + 2} differs"


# ---------------------------------------------------------------------------
# agreement with the project's own yardsticks
# ---------------------------------------------------------------------------

def _oracle_act(act, z, res):
    from mine_amd.ops.bn import _act_eager
    if act == "add_relu":
        return F.relu(z + res)
    return _act_eager(act, z)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", PARITY_CASES, ids=_id)
def test_module_parity_deterministic(act, case, restore_mode):
    """tests/test_bn_stream.py::test_module_parity inside
    `with deterministic():`, plus the running statistics after the step."""
    from mine_amd.ops import deterministic
    from mine_amd.ops.bn import FusedBNAct

    dtype, (B, C, H, W) = case
    M = B * H * W
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
    with deterministic():
        y = m(x, r) if act == "add_relu" else m(x)
    assert y.dtype == dtype
    # backward after the block: the graph keeps the mode it was built in
    (y.float() * gy.to(DEV)).sum().backward()

    xr = x0.to(dtype).float().requires_grad_(True)
    rr = r0.to(dtype).float().requires_grad_(True)
    gyr = gy.to(dtype).float()
    wr = m.weight.detach().cpu().clone().requires_grad_(True)
    br = m.bias.detach().cpu().clone().requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    zr = torch.batch_norm(xr, wr, br, rm, rv, True, 0.1, 1e-5, False)
    yr = _oracle_act(act, zr, rr)
    (yr * gyr).sum().backward()

    tol = _tol(dtype)
    torch.testing.assert_close(y.float().cpu(), yr.detach(), **tol)
    torch.testing.assert_close(x.grad.float().cpu(), xr.grad, **tol)
    if act == "add_relu":
        torch.testing.assert_close(r.grad.float().cpu(), rr.grad, **tol)
    torch.testing.assert_close(m.weight.grad.cpu(), wr.grad, **PTOL)
    torch.testing.assert_close(m.bias.grad.cpu(), br.grad, **PTOL)

    torch.testing.assert_close(m.running_mean.cpu(), rm, rtol=1e-5,
                               atol=1e-5)
    if M == 1:
        # torch.batch_norm's unbiased variance of one sample is 0/0 = NaN;
        # the kernels keep the biased variance (0) there, as
        # bn_finalize_kernel always has: 0.9 * 1 + 0.1 * 0
        assert torch.isnan(rv).all()
        rv = torch.full((C,), 0.9)
    torch.testing.assert_close(m.running_var.cpu(), rv, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", PARITY_CASES, ids=_id)
def test_sums_match_default_mode(case):
    dtype, (B, C, H, W) = case
    ext = _ext()
    M = B * H * W
    g = torch.Generator().manual_seed(46)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    for mb in (0, 1, 3):
        torch.testing.assert_close(
            ext.bn_sums(x, M, C, mb, deterministic=True),
            ext.bn_sums(x, M, C, mb), rtol=1e-5, atol=1e-5)
    # finalize fused into the finishing kernel vs. the stand-alone one
    empty = torch.empty(0, device=DEV)
    mean_d, invstd_d = ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1, 0,
                                    deterministic=True)
    mean, invstd = ext.bn_stats(x, M, C, empty, empty, 1e-5, 0.1)
    torch.testing.assert_close(mean_d, mean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(invstd_d, invstd, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("K", [16, 24])
def test_join_matches_default_mode(K):
    ext = _ext()
    B, S, H, W = 2, 3, 5, 7
    g = torch.Generator().manual_seed(34)
    y_dec = torch.randn(B * S * H * W * K, generator=g).to(DEV, BF16)
    y_base = torch.randn(B * H * W * K, generator=g).to(DEV, BF16)
    bias = torch.randn(B * S * K, generator=g).to(DEV, BF16)
    for mb in (0, 1, 3):
        x, sums = ext.bn_join_stats(y_dec, y_base, bias, B, S, H * W, K, mb)
        x_d, sums_d = ext.bn_join_stats(y_dec, y_base, bias, B, S, H * W, K,
                                        mb, deterministic=True)
        assert torch.equal(x_d, x)
        torch.testing.assert_close(sums_d, sums, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------
# igemm: split-K forward / data gradient and the weight gradient
# ---------------------------------------------------------------------------

IGEMM_SHAPES = [
    # (B, C, H, W, K, R, stride, pad, reflect)
    (1, 64, 8, 8, 16, 3, 1, 1, False),       # one block, splitz = 4
    (4, 128, 16, 24, 128, 3, 2, 1, False),   # splitz = 9, stride 2
    (4, 96, 10, 14, 40, 3, 1, 1, True),      # reflect, K % 16 != 0
    (4, 64, 16, 24, 256, 1, 1, 0, False),    # does not split
]


def _conv_ref(xq, wq, bq, R, stride, pad, reflect):
    if reflect:
        return F.conv2d(F.pad(xq, ((R - 1) // 2,) * 4, mode="reflect"), wq, bq)
    return F.conv2d(xq, wq, bq, stride=stride, padding=pad)


def _conv_run(x0, w0, b0, gy0, stride, pad, reflect):
    from mine_amd.ops.conv_general import conv2d_mfma
    x = _cl(x0, BF16).requires_grad_(True)
    w = w0.to(DEV).requires_grad_(True)
    b = b0.to(DEV).requires_grad_(True)
    y = conv2d_mfma(x, w, b, stride=stride, padding=pad, reflect=reflect)
    assert y.dtype == BF16
    y.backward(_cl(gy0, BF16))
    return [y.detach(), x.grad, w.grad, b.grad]


@pytest.mark.parametrize("shape", IGEMM_SHAPES,
                         ids=["x".join(map(str, s[:7])) for s in IGEMM_SHAPES])
def test_igemm_exact_on_integers(shape, restore_mode):
    from mine_amd.ops import deterministic

    B, C, H, W, K, R, stride, pad, reflect = shape
    x0 = _ints((B, C, H, W), -1, 1, 51).float()
    w0 = _ints((K, C, R, R), -1, 1, 52).float()
    b0 = _ints((K,), -2, 2, 53).float()

    xq = x0.clone().requires_grad_(True)
    wq = w0.clone().requires_grad_(True)
    bq = b0.clone().requires_grad_(True)
    yr = _conv_ref(xq, wq, bq, R, stride, pad, reflect)
    gy0 = _ints(tuple(yr.shape), -1, 1, 54).float()
    yr.backward(gy0)
    # exactly representable: y and dx in bf16, dw and db in fp32 partials
    assert yr.abs().max() <= 256
    assert xq.grad.abs().max() <= 256
    assert wq.grad.abs().max() < 1 << 24
    assert bq.grad.abs().max() < 1 << 24

    with deterministic():
        y, gx, gw, gb = _conv_run(x0, w0, b0, gy0, stride, pad, reflect)
    assert torch.equal(y.float().cpu(), yr.detach())
    assert torch.equal(gx.float().cpu(), xq.grad)
    assert torch.equal(gw.cpu(), wq.grad)
    assert torch.equal(gb.cpu(), bq.grad)


@pytest.mark.parametrize("shape", IGEMM_SHAPES,
                         ids=["x".join(map(str, s[:7])) for s in IGEMM_SHAPES])
def test_igemm_repeatable(shape, restore_mode):
    from mine_amd.ops import deterministic

    B, C, H, W, K, R, stride, pad, reflect = shape
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(B, C, H, W, generator=g)
    w0 = torch.randn(K, C, R, R, generator=g) * (0.5 / R)
    b0 = torch.randn(K, generator=g) * 0.1
    P = H if reflect else (H + 2 * pad - R) // stride + 1
    Q = W if reflect else (W + 2 * pad - R) // stride + 1
    gy0 = torch.randn(B, K, P, Q, generator=g)

    with deterministic():
        first = _conv_run(x0, w0, b0, gy0, stride, pad, reflect)
        for i in range(9):
            again = _conv_run(x0, w0, b0, gy0, stride, pad, reflect)
            for name, u, v in zip(("y", "x.grad", "w.grad", "b.grad"),
                                  again, first):
                assert torch.equal(u, v), f"{name}: run {i + 2} differs"
    if shape == IGEMM_SHAPES[3]:
        # no split-K here: the forward and data gradient are the default
        # mode's kernels and must match them bit for bit
        default = _conv_run(x0, w0, b0, gy0, stride, pad, reflect)
        assert torch.equal(default[0], first[0])
        assert torch.equal(default[1], first[1])


# ---------------------------------------------------------------------------
# network level
# ---------------------------------------------------------------------------

def test_network_bit_reproducible(restore_mode):
    """Backbone + decoder as SynthesisTask builds them (bf16,
    channels_last, 128x192, 8 planes, batch 2, training.deterministic):
    two forwards from the same weights, input and disparities are
    bit-identical at all four scales, and so are two backwards from one
    fixed upstream gradient — every parameter gradient and every BN
    running statistic."""
    from mine_amd.config import default_config
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import is_deterministic

    B, S, H, W = 2, 8, 128, 192
    cfg = default_config(**{
        "data.name": "synthetic", "data.img_h": H, "data.img_w": W,
        "mpi.num_bins_coarse": S, "data.per_gpu_batch_size": B,
        "data.visible_point_count": 32, "data.num_workers": 0,
        "training.deterministic": True,
    })
    torch.manual_seed(61)
    task = SynthesisTask(cfg, device=DEV)
    assert is_deterministic()
    assert task.amp_dtype == BF16 and task.channels_last
    nets = [task.backbone, task.decoder]
    state = [{k: v.clone() for k, v in n.state_dict().items()} for n in nets]

    g = torch.Generator().manual_seed(62)
    src = torch.rand(B, 3, H, W, generator=g).to(DEV).contiguous(
        memory_format=torch.channels_last)
    disparity = torch.linspace(1.0, 0.05, S).repeat(B, 1).to(DEV)
    ups = None

    def run():
        nonlocal ups
        for n, sd in zip(nets, state):
            n.load_state_dict(sd)
            n.zero_grad(set_to_none=True)
        outs = task.mpi_predictor(src, disparity)
        assert len(outs) == 4
        if ups is None:
            ups = [torch.randn(o.shape, generator=g).to(DEV) for o in outs]
        torch.autograd.backward(outs, ups)
        grads = {f"{i}.{k}": p.grad.detach().clone()
                 for i, n in enumerate(nets)
                 for k, p in n.named_parameters() if p.grad is not None}
        bufs = {f"{i}.{k}": b.detach().clone() for i, n in enumerate(nets)
                for k, b in n.named_buffers()}
        return [o.detach().clone() for o in outs], grads, bufs

    outs1, grads1, bufs1 = run()
    outs2, grads2, bufs2 = run()
    for s in range(4):
        assert torch.equal(outs1[s], outs2[s]), f"MPI scale {s} differs"
    assert grads1 and grads1.keys() == grads2.keys()
    bad = [k for k in grads1 if not torch.equal(grads1[k], grads2[k])]
    assert not bad, f"{len(bad)} of {len(grads1)} gradients differ: {bad[:8]}"
    assert any("running_mean" in k for k in bufs1)
    bad = [k for k in bufs1 if not torch.equal(bufs1[k], bufs2[k])]
    assert not bad, f"buffers differ: {bad[:8]}"
