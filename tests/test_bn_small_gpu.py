"""Small-layer BatchNorm path (ext._bn): a reduction that stores G partial
rows and a consumer that adds them in its prologue, two launches per
direction.

Exactness tests use integer data in [-4, 4], for which every fp32
summation order is exact (tests/test_deterministic_gpu.py): the sums can
only be wrong by a dropped or doubled partial, and with exact sums the new
forward must reproduce bn_finalize + bn_act_fwd bit for bit. On random
data the new consumers are compared bit for bit with the existing ones fed
with the statistics the new path returned (one shared body), and with
themselves across consumer grids (one sum for all workgroups). The module
tests use the tolerances of tests/test_bn_stream.py.

Shapes: 2x64x9x11 (cgv 8, M no multiple of the rows per block), 3x256x7x9
(cgv 32), 1x2048x3x4 (four channel chunks, M = 12), 2x24x5x7 (Cv = 3: idle
lanes through the prologue barrier), 2x12x9x11 (V = 1 for 16-bit, V = 4 for
fp32), 1x12x1x1 (M = 1, variance 0).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = ["none", "relu", "lrelu", "elu", "add_relu"]
ACT_ID = {a: i for i, a in enumerate(ACTS)}
SHAPES = [(2, 64, 9, 11), (3, 256, 7, 9), (1, 2048, 3, 4), (2, 24, 5, 7),
          (2, 12, 9, 11), (1, 12, 1, 1)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CASES = [(d, s) for d in DTYPES for s in SHAPES]
GRIDS = [(r, c) for r in (0, 1, 3) for c in (0, 1, 3)]  # (reduce, consumer)
EPS, MOM = 1e-5, 0.1


def _id(case):
    d, s = case
    return str(d).split(".")[-1] + "-" + "x".join(map(str, s))


def _ext():
    from mine_amd.ops.backend import get_extension
    return get_extension(required=True)   # missing is an error, not a skip


def _tol(dtype):   # tests/test_bn_stream.py: _tol, PTOL
    return dict(rtol=1e-2, atol=1e-2) if dtype == torch.bfloat16 else \
        dict(rtol=1e-4, atol=1e-4)


PTOL = dict(rtol=1e-4, atol=1e-3)


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g)


def _params(C, seed, beta_shift=0.0):
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2 + beta_shift).to(DEV)
    return gamma, beta


def _running(C):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(C, generator=g).to(DEV),
            (torch.rand(C, generator=g) + 0.5).to(DEV),
            torch.tensor(7, device=DEV))


def _none(dtype=torch.float32):
    return torch.empty(0, device=DEV, dtype=dtype)


def _new_fwd(x, res, gamma, beta, M, C, act, rm, rv, nbt, mbr=0, mbc=0,
             ws=None):
    bn = _ext()._bn
    if ws is None:
        ws = bn.stats_partials(x, M, C, mbr)
    return bn.act_fwd_ws(x, res, ws, gamma, beta, M, C, act, rm, rv, nbt,
                         EPS, MOM, mbr, mbc)


def _new_bwd(x, res, gy, mean, invstd, gamma, beta, M, C, act, mbr=0, mbc=0,
             ws=None):
    bn = _ext()._bn
    if ws is None:
        ws = bn.bwd_reduce_partials(x, res, gy, mean, invstd, gamma, beta, M,
                                    C, act, mbr)
    return bn.act_bwd_dx_ws(x, res, gy, mean, invstd, gamma, beta, ws, M, C,
                            act, mbr, mbc)


def test_plan_on_the_flagship_shapes():
    """The plan is a pure host function: bounded grids, and the size rule
    keeps the decoder's big layers off the path."""
    bn = _ext()._bn
    for (N, C, H, W) in [(4, 64, 128, 192), (4, 256, 64, 96),
                         (4, 2048, 8, 12), (4, 512, 8, 12)]:
        small, G, cgv, gx = bn.small_plan(N * H * W, C, torch.bfloat16)
        assert small
        assert 1 <= G <= 4096 and 1 <= gx <= 4096
        assert cgv in (1, 2, 4, 8, 16, 32, 64)
    for (N, C, H, W) in [(256, 16, 256, 384), (256, 256, 16, 24)]:
        assert not bn.small_plan(N * H * W, C, torch.bfloat16)[0]


# ---------------------------------------------------------------------------
# exact sums
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_exact_on_integers(case):
    dtype, (B, C, H, W) = case
    ext = _ext()
    M = B * H * W
    xi = _ints((M, C), 41)
    exact = torch.cat((xi.sum(0), (xi * xi).sum(0))).float().to(DEV)
    x = xi.reshape(-1).to(DEV, dtype)
    r = _ints((M, C), 44).reshape(-1).to(DEV, dtype)
    gamma, beta = _params(C, 3)
    rm_ref, rv_ref, _ = _running(C)
    mean_ref, invstd_ref = ext.bn_finalize(exact, M, C, rm_ref, rv_ref, EPS,
                                           MOM)
    for act in ACTS:
        res = r if act == "add_relu" else _none(dtype)
        y_ref = ext.bn_act_fwd(x, res, mean_ref, invstd_ref, gamma, beta, M,
                               C, ACT_ID[act])
        for mbr, mbc in GRIDS:
            rm, rv, nbt = _running(C)
            y, mean, invstd = _new_fwd(x, res, gamma, beta, M, C,
                                       ACT_ID[act], rm, rv, nbt, mbr, mbc)
            where = f"{act} reduce={mbr} consumer={mbc}"
            assert torch.equal(mean, mean_ref), where
            assert torch.equal(invstd, invstd_ref), where
            assert torch.equal(rm, rm_ref), where
            assert torch.equal(rv, rv_ref), where
            assert torch.equal(y, y_ref), where
            assert int(nbt) == 8, where


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_backward_dbeta_exact_on_integers(case):
    """beta = 100 puts every pre-activation above zero (|xhat| < sqrt(M),
    |res| <= 4), so act' = 1 and dbeta is the plain sum of gy for every
    activation."""
    dtype, (B, C, H, W) = case
    M = B * H * W
    gi = _ints((M, C), 42)
    exact = gi.sum(0).float().to(DEV)
    g = torch.Generator().manual_seed(43)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = gi.reshape(-1).to(DEV, dtype)
    r = _ints((M, C), 44).reshape(-1).to(DEV, dtype)
    gamma, beta = _params(C, 3, beta_shift=100.0)
    _, mean, invstd = _new_fwd(x, _none(dtype), gamma, beta, M, C, 0,
                               _none(), _none(), _none())
    for act in ACTS:
        res = r if act == "add_relu" else _none(dtype)
        for mbr, mbc in GRIDS:
            _, _, red = _new_bwd(x, res, gy, mean, invstd, gamma, beta, M, C,
                                 ACT_ID[act], mbr, mbc)
            assert red.shape == (2 * C,)
            assert torch.equal(red[:C], exact), \
                f"{act} reduce={mbr} consumer={mbc}"


# ---------------------------------------------------------------------------
# shared bodies, one sum for all workgroups
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_id)
def test_consumers_share_the_bodies_and_the_sum(case):
    dtype, (B, C, H, W) = case
    ext = _ext()
    bn = ext._bn
    M = B * H * W
    g = torch.Generator().manual_seed(31)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    r = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = torch.randn(M * C, generator=g).to(DEV, dtype)
    gamma, beta = _params(C, 3)
    # the existing kernels run on the plan's consumer grid too: a thread
    # then owns the same rows in both
    gx = bn.small_plan(M, C, dtype)[3]
    for act in ACTS:
        a = ACT_ID[act]
        res = r if act == "add_relu" else _none(dtype)
        for mbr in (0, 1, 3):
            ws = bn.stats_partials(x, M, C, mbr)
            first = None
            # two calls on the plan's grid, then the forced consumer grids
            for mbc in (0, 0, 1, 3):
                y, mean, invstd = _new_fwd(x, res, gamma, beta, M, C, a,
                                           _none(), _none(), _none(), mbr,
                                           mbc, ws=ws)
                if first is None:
                    first = (y, mean, invstd)
                    y_old = ext.bn_act_fwd(x, res, mean, invstd, gamma, beta,
                                           M, C, a, gx)
                    assert torch.equal(y, y_old), (act, mbr)
                for got, want in zip((y, mean, invstd), first):
                    assert torch.equal(got, want), (act, mbr, mbc)
            y, mean, invstd = first
            wsb = bn.bwd_reduce_partials(x, res, gy, mean, invstd, gamma,
                                         beta, M, C, a, mbr)
            first = None
            for mbc in (0, 0, 1, 3):
                dx, dres, red = _new_bwd(x, res, gy, mean, invstd, gamma,
                                         beta, M, C, a, mbr, mbc, ws=wsb)
                if first is None:
                    first = (dx, dres, red)
                    dx_old, dres_old = ext.bn_act_bwd_dx(
                        x, res, gy, mean, invstd, gamma, beta, red, M, C, a,
                        M, gx)
                    assert torch.equal(dx, dx_old), (act, mbr)
                    assert torch.equal(dres, dres_old), (act, mbr)
                for got, want in zip((dx, dres, red), first):
                    assert torch.equal(got, want), (act, mbr, mbc)
            # a second reduction of the same input gives the same partials
            assert torch.equal(
                wsb, bn.bwd_reduce_partials(x, res, gy, mean, invstd, gamma,
                                            beta, M, C, a, mbr)), (act, mbr)
            assert torch.equal(ws, bn.stats_partials(x, M, C, mbr)), (act, mbr)


def test_reduction_chunk_width_does_not_change_the_layout():
    """The reduction's cgv is free: narrower chunks, same (G,2,C) sums."""
    bn = _ext()._bn
    B, C, H, W = 3, 256, 7, 9
    M = B * H * W
    x = _ints((M, C), 41).reshape(-1).to(DEV, torch.bfloat16)
    want = bn.stats_partials(x, M, C, 3).sum(0)
    for cgv in (1, 4, 8, 32):
        ws = bn.stats_partials(x, M, C, 3, cgv)
        assert ws.shape == (3, 2, C)
        assert torch.equal(ws.sum(0), want), cgv


# ---------------------------------------------------------------------------
# single owner
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 2048, 3, 4), (3, 256, 7, 9)],
                         ids=lambda s: "x".join(map(str, s)))
def test_single_owner_of_buffers_and_counter(shape):
    """Several blocks in x (forced 3) and, at C = 2048, four in y."""
    B, C, H, W = shape
    M = B * H * W
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gamma, beta = _params(C, 3)
    rm, rv, nbt = _running(C)
    rm0, rv0 = rm.clone(), rv.clone()
    _, mean, invstd = _new_fwd(x, _none(dtype), gamma, beta, M, C, 1, rm, rv,
                               nbt, 3, 3)
    assert int(nbt) == 8
    var = 1.0 / invstd.double() ** 2 - EPS
    unbiased = var * M / max(M - 1, 1)
    torch.testing.assert_close(
        rm.double(), rm0.double() + MOM * (mean.double() - rm0.double()),
        rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(
        rv.double(), rv0.double() + MOM * (unbiased - rv0.double()),
        rtol=1e-4, atol=1e-5)
    _new_fwd(x, _none(dtype), gamma, beta, M, C, 1, rm, rv, nbt, 3, 3)
    assert int(nbt) == 9
    # no running tensors, no counter: the statistics come back, nothing else
    rm1, rv1 = rm.clone(), rv.clone()
    _, mean2, invstd2 = _new_fwd(x, _none(dtype), gamma, beta, M, C, 1,
                                 _none(), _none(), _none(), 3, 3)
    assert torch.equal(mean2, mean) and torch.equal(invstd2, invstd)
    assert torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nbt) == 9


# ---------------------------------------------------------------------------
# module
# ---------------------------------------------------------------------------

def _cl(t, dtype):
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _run_module(shape, dtype, act, how, monkeypatch, momentum=0.1):
    """One train-mode forward + backward; `how` is "small", "old"
    (MINE_BN_COMPACT=0) or "fallback". Returns what the issue compares."""
    from mine_amd.ops import bn as bn_mod

    B, C, H, W = shape
    g = torch.Generator().manual_seed(31)
    x0 = torch.randn(B, C, H, W, generator=g)
    r0 = torch.randn(B, C, H, W, generator=g)
    gy = torch.randn(B, C, H, W, generator=g)
    m = bn_mod.FusedBNAct(C, act=act, momentum=momentum).to(DEV).train()
    with torch.no_grad():
        m.weight.copy_(torch.rand(C, generator=g) + 0.5)
        m.bias.copy_(torch.randn(C, generator=g) * 0.2)
    x = _cl(x0, dtype).requires_grad_(True)
    r = _cl(r0, dtype).requires_grad_(True) if act == "add_relu" else None
    monkeypatch.setenv("MINE_BN_COMPACT", "0" if how == "old" else "1")
    taken = []
    real = bn_mod._BNActSmallFn.apply
    monkeypatch.setattr(bn_mod._BNActSmallFn, "apply",
                        lambda *a: (taken.append(1), real(*a))[1])
    if how == "fallback":
        y = m._fallback(x, r)
    else:
        y = m(x, r) if act == "add_relu" else m(x)
    (y.float() * _cl(gy, torch.float32)).sum().backward()
    out = dict(y=y.detach().float(), dx=x.grad.float(),
               dgamma=m.weight.grad.clone(), dbeta=m.bias.grad.clone(),
               rm=m.running_mean.clone(), rv=m.running_var.clone(),
               nbt=int(m.num_batches_tracked))
    if act == "add_relu":
        out["dres"] = r.grad.float()
    return out, bool(taken)


@pytest.mark.parametrize("act", ["relu", "add_relu"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", [(2, 64, 9, 11), (3, 256, 7, 9)],
                         ids=lambda s: "x".join(map(str, s)))
def test_module_takes_the_path_and_agrees(shape, dtype, act, monkeypatch):
    new, took = _run_module(shape, dtype, act, "small", monkeypatch)
    assert took
    old, took_old = _run_module(shape, dtype, act, "old", monkeypatch)
    assert not took_old
    ref, _ = _run_module(shape, dtype, act, "fallback", monkeypatch)
    tol = _tol(dtype)
    for other in (old, ref):
        for k in ("y", "dx") + (("dres",) if act == "add_relu" else ()):
            torch.testing.assert_close(new[k], other[k], **tol,
                                       msg=lambda s: f"{k}: {s}")
        for k in ("dgamma", "dbeta"):
            torch.testing.assert_close(new[k], other[k], **PTOL,
                                       msg=lambda s: f"{k}: {s}")
        # F.batch_norm (the fallback) does not count batches itself
        assert new["nbt"] == 1 and old["nbt"] == 1
        torch.testing.assert_close(new["rm"], other["rm"], **PTOL)
        torch.testing.assert_close(new["rv"], other["rv"], **PTOL)


def test_module_keeps_the_old_path_where_it_must(monkeypatch):
    from mine_amd.ops import bn as bn_mod
    shape, dtype = (2, 64, 9, 11), torch.bfloat16
    # momentum=None: the cumulative average needs the counter on the host
    out, took = _run_module(shape, dtype, "relu", "small", monkeypatch,
                            momentum=None)
    assert not took and out["nbt"] == 1
    # supplied sums
    B, C, H, W = shape
    m = bn_mod.FusedBNAct(C, act="relu").to(DEV).train()
    x = _cl(torch.randn(B, C, H, W), dtype)
    M = B * H * W
    sums = _ext().bn_sums(x.permute(0, 2, 3, 1).reshape(-1), M, C)
    monkeypatch.setattr(bn_mod._BNActSmallFn, "apply", None)  # must not run
    y = m(x, sums=sums)
    assert int(m.num_batches_tracked) == 1
    torch.testing.assert_close(y.float(), m._fallback(x, None).float(),
                               **_tol(dtype))
    # a shape the plan refuses (18.9 MB)
    B, C, H, W = 1, 8, 768, 768
    assert not _ext()._bn.small_plan(B * H * W, C, torch.float32)[0]
    m = bn_mod.FusedBNAct(C, act="relu").to(DEV).train()
    m(_cl(torch.randn(B, C, H, W), torch.float32))
    m(_cl(torch.randn(B, C, H, W), torch.float32))
    assert int(m.num_batches_tracked) == 2


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def _good_args(binding):
    """Valid keyword arguments of one _bn binding at 2x64x9x11 bf16."""
    bn = _ext()._bn
    B, C, H, W = 2, 64, 9, 11
    M = B * H * W
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M * C, generator=g).to(DEV, dtype)
    gy = torch.randn(M * C, generator=g).to(DEV, dtype)
    gamma, beta = _params(C, 3)
    rm, rv, nbt = _running(C)
    if binding == "stats_partials":
        return dict(x=x, M=M, C=C, max_blocks=3)
    ws = bn.stats_partials(x, M, C, 3)
    fwd = dict(x=x, res=_none(dtype), ws=ws, gamma=gamma, beta=beta, M=M, C=C,
               act=1, running_mean=rm, running_var=rv,
               num_batches_tracked=nbt, eps=EPS, momentum=MOM,
               max_blocks_reduce=3, max_blocks=2)
    if binding == "act_fwd_ws":
        return fwd
    _, mean, invstd = bn.act_fwd_ws(**fwd)
    red = dict(x=x, res=_none(dtype), gy=gy, mean=mean, invstd=invstd,
               gamma=gamma, beta=beta, M=M, C=C, act=1, max_blocks=3)
    if binding == "bwd_reduce_partials":
        return red
    wsb = bn.bwd_reduce_partials(**red)
    del red["max_blocks"]
    return dict(red, ws=wsb, max_blocks_reduce=3, max_blocks=2)


def _refusals(binding, args):
    """(label, changed arguments, text the message must hold)"""
    x, C = args["x"], args["C"]
    wide = torch.zeros(2 * x.numel(), device=DEV, dtype=x.dtype)[::2]
    cases = [
        ("x on the CPU", dict(x=x.cpu()), "x must be on the GPU"),
        ("int x", dict(x=x.int()), "x must be f32 or bf16 or fp16"),
        ("short x", dict(x=x[:-1].clone()),
         f"x must have {x.numel()} elements"),
        ("non-contiguous x", dict(x=wide), "x must be contiguous"),
    ]
    if "gamma" in args:
        cases += [
            ("bf16 gamma", dict(gamma=args["gamma"].bfloat16()),
             "gamma must be f32"),
            ("short beta", dict(beta=args["beta"][:-1].clone()),
             f"beta must have {C} elements"),
            ("fp16 res", dict(res=x.half()), "res must be bf16"),
        ]
    if "ws" in args:
        ws = args["ws"]
        cases += [
            ("workspace of another G", dict(ws=ws[:2].clone()),
             f"ws must have {3 * 2 * C} elements"),
            ("workspace rows and G disagree", dict(max_blocks_reduce=2),
             f"ws must have {2 * 2 * C} elements"),
            ("f64 workspace", dict(ws=ws.double()), "ws must be f32"),
        ]
    if "gy" in args:
        cases += [("short gy", dict(gy=args["gy"][:-1].clone()),
                   f"gy must have {x.numel()} elements"),
                  ("short mean", dict(mean=args["mean"][:-1].clone()),
                   f"mean must have {C} elements")]
    if binding == "act_fwd_ws":
        cases += [
            ("int32 counter",
             dict(num_batches_tracked=args["num_batches_tracked"].int()),
             "num_batches_tracked must be int64"),
            ("running_var alone", dict(running_mean=_none()),
             "running_mean and running_var go together"),
        ]
    return cases


@pytest.mark.parametrize("binding", ["stats_partials", "act_fwd_ws",
                                     "bwd_reduce_partials", "act_bwd_dx_ws"])
def test_binding_refusals(binding):
    args = _good_args(binding)
    fn = getattr(_ext()._bn, binding)
    fn(**args)                                  # the unchanged call runs
    nbt = args.get("num_batches_tracked")
    count = None if nbt is None else int(nbt)
    for label, change, text in _refusals(binding, args):
        bad = dict(args)
        bad.update(change)
        with pytest.raises(RuntimeError) as err:
            fn(**bad)
        msg = str(err.value).splitlines()[0]
        assert msg.startswith(binding + ": "), (label, msg)
        assert text in msg, (label, msg)
    if nbt is not None:                         # nothing was launched
        assert int(nbt) == count
