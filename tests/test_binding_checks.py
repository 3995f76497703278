"""Argument checks of the `_mine_hip` bindings (csrc/bindings.hip).

Every binding validates every tensor before it hands a pointer to a
launcher: on the GPU and on the first tensor's device, contiguous, dtype,
numel as the geometry implies. One table of (binding, builder of valid
arguments at the smallest legal shape) drives both parts:

  * without a GPU, every binding refuses its CPU arguments and names the
    first tensor;
  * on the GPU, every tensor argument is corrupted one way at a time and
    the error names that argument; afterwards the valid call still runs,
    and an empty tensor is accepted wherever it means "absent".

A launch that slipped through a missing check must still read allocated
memory only, so a corruption never shortens a tensor or narrows its dtype:
a wider dtype, the other 16-bit type, a non-contiguous view of equal numel
over a larger buffer, or one slice too many.

reflect_pad_fwd and upsample2x_fwd are pure copies and are compared
exactly with F.pad(mode="reflect") and repeat_interleave.
"""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
BF16, F16 = torch.bfloat16, torch.float16
I32, I64 = torch.int32, torch.int64
HALVES = (BF16, F16)


def _ext():
    from mine_amd.ops.backend import get_extension
    return get_extension(required=True)


def _vals(dev, dtype, *shape):
    """Small exactly representable values, no zeros."""
    n = 1
    for s in shape:
        n *= s
    v = (torch.arange(n) % 7 + 1).to(torch.float32) * 0.25
    return v.reshape(shape).to(dev, dtype)


def _eye(dev, *lead):
    return torch.eye(3).expand(*lead, 3, 3).contiguous().to(dev)


# ---------------------------------------------------------------------------
# builders: device -> ordered (argument name -> value). Tensor names are the
# bindings' own, as the error messages spell them.
# ---------------------------------------------------------------------------

B, S, H, W = 1, 2, 4, 8           # mpi (1, 2, 4, 8, 4)


def _mpi_parts(dev):
    return dict(
        mpi=_vals(dev, F32, B, S, H, W, 4),
        depths=torch.tensor([[1.0, 2.0]]).to(dev),
        eye_bs=_eye(dev, B, S), eye_b=_eye(dev, B),
        tvec=torch.zeros(B, 3).to(dev),
        img=_vals(dev, F32, B, H, W, 3),
        g_rgb=_vals(dev, F32, B, 3, H, W),
        g_depth=_vals(dev, F32, B, 1, H, W))


def b_src_fwd(dev):
    p = _mpi_parts(dev)
    return OrderedDict(mpi=p["mpi"], depths=p["depths"], kinv=p["eye_b"],
                       img=p["img"], bg_inf=False, alpha=False)


def b_src_bwd(dev):
    p = _mpi_parts(dev)
    return OrderedDict(mpi=p["mpi"], depths=p["depths"], kinv=p["eye_b"],
                       img=p["img"], bg_inf=False, alpha=False,
                       g_rgb=p["g_rgb"], g_depth=p["g_depth"],
                       g_blend=_vals(dev, F32, B, S, H, W, 4))


def b_tgt_fwd(dev):
    p = _mpi_parts(dev)
    return OrderedDict(mpi=p["mpi"], hinv=p["eye_bs"], m=p["eye_b"],
                       tvec=p["tvec"], depths=p["depths"], bg_inf=False,
                       alpha=False)


def b_tgt_bwd(dev):
    p = _mpi_parts(dev)
    return OrderedDict(mpi=p["mpi"], hinv=p["eye_bs"], hfwd=p["eye_bs"].clone(),
                       m=p["eye_b"], tvec=p["tvec"], depths=p["depths"],
                       bg_inf=False, alpha=False, g_rgb=p["g_rgb"],
                       g_depth=p["g_depth"], mode=1,
                       workspace=torch.empty_like(p["mpi"]))


def b_tgt_collect(dev):
    p = _mpi_parts(dev)
    return OrderedDict(payload=p["mpi"], hinv=p["eye_bs"],
                       hfwd=p["eye_bs"].clone())


def b_ssim_fwd(dev):
    return OrderedDict(img1=_vals(dev, F32, 1, 1, 12, 12),
                       img2=_vals(dev, F32, 1, 1, 12, 12).flip(3).contiguous(),
                       det=False)


def b_ssim_bwd(dev):
    a = b_ssim_fwd(dev)
    return OrderedDict(img1=a["img1"], img2=a["img2"],
                       gscale=torch.tensor(1.0).to(dev))


def b_eav2_fwd(dev):
    return OrderedDict(disp=_vals(dev, F32, 1, 1, 12, 12),
                       img=_vals(dev, F32, 1, 3, 12, 12),
                       mean_d=torch.ones(1).to(dev), det=False)


def b_eav2_bwd(dev):
    a = b_eav2_fwd(dev)
    return OrderedDict(disp=a["disp"], img=a["img"], mean_d=a["mean_d"],
                       gl=torch.ones(1).to(dev), det=False)


def b_gather(dev):
    return OrderedDict(grad_out=_vals(dev, F32, 1, 2, 3),
                       idx=torch.tensor([[0, 5, 5]], dtype=I64).to(dev),
                       HW=16)


PAD = dict(N=1, H=4, W=4, C=8)


def b_pad_fwd(dev, dtype=BF16):
    return OrderedDict(**{"in": _vals(dev, dtype, 1 * 4 * 4 * 8)}, **PAD,
                       pad=1)


def b_pad_bwd(dev, dtype=BF16):
    return OrderedDict(gout=_vals(dev, dtype, 1 * 6 * 6 * 8), **PAD, pad=1)


def b_up_fwd(dev, dtype=BF16):
    return OrderedDict(**{"in": _vals(dev, dtype, 1 * 4 * 4 * 8)}, **PAD)


def b_up_bwd(dev, dtype=BF16):
    return OrderedDict(gout=_vals(dev, dtype, 1 * 8 * 8 * 8), **PAD)


M, C = 8, 8                        # BN


def _bn_parts(dev, dtype):
    return dict(x=_vals(dev, dtype, M * C),
                res=_vals(dev, dtype, M * C).flip(0).contiguous(),
                gy=_vals(dev, dtype, M * C),
                mean=_vals(dev, F32, C), invstd=_vals(dev, F32, C),
                gamma=_vals(dev, F32, C), beta=_vals(dev, F32, C))


def b_bn_sums(dev, dtype=BF16):
    return OrderedDict(x=_vals(dev, dtype, M * C), M=M, C=C, max_blocks=0,
                       deterministic=False)


def b_bn_finalize(dev):
    return OrderedDict(sums=_vals(dev, F32, 2 * C) + 8.0, M=M, C=C,
                       running_mean=torch.zeros(C).to(dev),
                       running_var=torch.ones(C).to(dev), eps=1e-5,
                       momentum=0.1)


def b_bn_stats(dev, dtype=BF16):
    return OrderedDict(x=_vals(dev, dtype, M * C), M=M, C=C,
                       running_mean=torch.zeros(C).to(dev),
                       running_var=torch.ones(C).to(dev), eps=1e-5,
                       momentum=0.1, max_blocks=0, deterministic=False)


def b_bn_join(dev, dtype=BF16):
    Bj, Sj, HW = 1, 2, 4
    return OrderedDict(y_dec=_vals(dev, dtype, Bj * Sj * HW * C),
                       y_base=_vals(dev, dtype, Bj * HW * C),
                       bias=_vals(dev, dtype, Bj * Sj * C), B=Bj, S=Sj, HW=HW,
                       C=C, max_blocks=0, deterministic=False)


def b_bn_act_fwd(dev, dtype=BF16):
    p = _bn_parts(dev, dtype)
    return OrderedDict(x=p["x"], res=p["res"], mean=p["mean"],
                       invstd=p["invstd"], gamma=p["gamma"], beta=p["beta"],
                       M=M, C=C, act=4, max_blocks=0)


def b_bn_bwd_reduce(dev, dtype=BF16):
    p = _bn_parts(dev, dtype)
    return OrderedDict(x=p["x"], res=p["res"], gy=p["gy"], mean=p["mean"],
                       invstd=p["invstd"], gamma=p["gamma"], beta=p["beta"],
                       M=M, C=C, act=4, max_blocks=0, deterministic=False)


def b_bn_bwd_dx(dev, dtype=BF16):
    p = _bn_parts(dev, dtype)
    return OrderedDict(x=p["x"], res=p["res"], gy=p["gy"], mean=p["mean"],
                       invstd=p["invstd"], gamma=p["gamma"], beta=p["beta"],
                       red=_vals(dev, F32, 2 * C), M=M, C=C, act=4, M_norm=M,
                       max_blocks=0)


def b_bn_bwd(dev, dtype=BF16):
    p = _bn_parts(dev, dtype)
    return OrderedDict(x=p["x"], res=p["res"], gy=p["gy"], mean=p["mean"],
                       invstd=p["invstd"], gamma=p["gamma"], beta=p["beta"],
                       M=M, C=C, act=4, deterministic=False)


def b_head_fwd(dev, dtype=BF16):
    return OrderedDict(z=_vals(dev, dtype, 8 * 4), N=8, alpha=False)


def b_head_bwd(dev, dtype=BF16):
    return OrderedDict(z=_vals(dev, dtype, 8 * 4), gout=_vals(dev, F32, 8 * 4),
                       N=8, alpha=False)


CN, CH, CW, CC, CK = 1, 4, 8, 16, 16   # conv3x3


def b_conv_fwd(dev, dtype=BF16):
    from mine_amd.ops.conv import pack_weights
    if torch.device(dev).type == "cuda":
        wp = pack_weights(_vals(dev, F32, CK, CC, 3, 3), dtype=dtype)
    else:  # the packed size of (K, C) = (16, 16): 1 k-tile x 5 chunks
        wp = _vals(dev, dtype, 1 * 5 * 64 * 8)
    return OrderedDict(x_flat=_vals(dev, dtype, CN * CH * CW * CC), wp=wp,
                       bias=_vals(dev, F32, CK),
                       out=torch.zeros(CN * CH * CW * CK).to(dev, dtype),
                       N=CN, H=CH, W=CW, C=CC, K=CK, pad_mode=0, src_h=CH,
                       src_w=CW, off=0, c_mem=0)


def b_conv_pack(dev):
    n_w = CK * CC * 9
    return OrderedDict(w_flat=_vals(dev, F32, n_w),
                       lut=(torch.arange(5 * 512) % (n_w + 1)).to(dev, I64),
                       dtype=None)


def b_wrw(dev, dtype=BF16):
    return OrderedDict(x_flat=_vals(dev, dtype, CN * CH * CW * CC),
                       gy_flat=_vals(dev, dtype, CN * CH * CW * CK), N=CN,
                       H=CH, W=CW, C=CC, K=CK, max_slabs=0)


# igemm 1x1: M = 8 pixels as one 2x4 image, C = K = 8
IG = OrderedDict(M=8, P=2, Q=4, K=8, Hs=2, Ws=4, C=8, R=1, S=1, SA=1, SB=1,
                 SD=0, SE=1, pad_mode=0, deterministic=False)


def b_pack_gather(dev):
    return OrderedDict(w=_vals(dev, F32, 64),
                       lut=(torch.arange(512) % 65 - 1).to(dev, I32),
                       dtype=None)


def b_igemm_fwd(dev, dtype=BF16):
    return OrderedDict(x_flat=_vals(dev, dtype, 8 * 8),
                       wp=_vals(dev, dtype, 512),   # 1 k-tile x 1 chunk
                       bias=_vals(dev, F32, 8), **IG)


def b_igemm_wrw(dev, dtype=BF16):
    return OrderedDict(x_flat=_vals(dev, dtype, 8 * 8),
                       gy_flat=_vals(dev, dtype, 8 * 8), **IG)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------

class Entry:
    """binding: attribute of the extension. any_float: the first tensor may
    also be f32, so only f64 is a wrong dtype for it. geometry: arguments
    whose own shape is the geometry, so one slice more is no corruption of
    them. strided: arguments taken by strides (any layout). absent: optional
    argument -> the other arguments to change with it."""

    def __init__(self, binding, build, over=None, any_float=False,
                 geometry=(), strided=(), absent=None, tag=""):
        self.binding, self.build, self.over = binding, build, over or {}
        self.any_float, self.geometry = any_float, set(geometry)
        self.strided, self.absent = set(strided), absent or {}
        self.id = binding + tag

    def args(self, dev):
        a = self.build(dev)
        a.update(self.over)
        return a

    def call(self, args):
        return getattr(_ext(), self.binding)(*args.values())


DET = dict(deterministic=True)
TABLE = [
    Entry("src_composite_fwd", b_src_fwd, absent={"img": {}}),
    Entry("src_composite_bwd", b_src_bwd,
          absent={"img": {}, "g_rgb": {}, "g_depth": {}, "g_blend": {}}),
    Entry("tgt_composite_fwd", b_tgt_fwd),
    Entry("tgt_composite_bwd", b_tgt_bwd,
          absent={"g_rgb": {}, "g_depth": {},
                  "hfwd": {"mode": 0, "workspace": None}}),
    Entry("tgt_composite_bwd", b_tgt_bwd, over={"mode": 2}, tag="-mode2"),
    Entry("tgt_collect", b_tgt_collect),
    Entry("ssim_fwd", b_ssim_fwd, geometry=["img1"]),
    Entry("ssim_fwd", b_ssim_fwd, over={"det": True}, geometry=["img1"],
          tag="-det"),
    Entry("ssim_bwd", b_ssim_bwd, geometry=["img1"]),
    Entry("reflect_pad_fwd", b_pad_fwd, any_float=True),
    Entry("reflect_pad_bwd", b_pad_bwd, any_float=True),
    Entry("bn_sums", b_bn_sums, any_float=True),
    Entry("bn_sums", b_bn_sums, over=DET, any_float=True, tag="-det"),
    Entry("bn_finalize", b_bn_finalize,
          absent={"running_mean": {"running_var": "absent"}}),
    Entry("bn_stats", b_bn_stats, any_float=True,
          absent={"running_mean": {"running_var": "absent"}}),
    Entry("bn_stats", b_bn_stats, over=DET, any_float=True, tag="-det",
          absent={"running_mean": {"running_var": "absent"}}),
    Entry("bn_join_stats", b_bn_join),
    Entry("bn_join_stats", b_bn_join, over=DET, tag="-det"),
    Entry("bn_act_fwd", b_bn_act_fwd, any_float=True,
          absent={"res": {"act": 1}}),
    Entry("bn_act_bwd_reduce", b_bn_bwd_reduce, any_float=True,
          absent={"res": {"act": 3}}),
    Entry("bn_act_bwd_reduce", b_bn_bwd_reduce, over=DET, any_float=True,
          tag="-det"),
    Entry("bn_act_bwd_dx", b_bn_bwd_dx, any_float=True,
          absent={"res": {"act": 2}}),
    Entry("bn_act_bwd", b_bn_bwd, any_float=True, absent={"res": {"act": 0}}),
    Entry("mpi_head_fwd", b_head_fwd, any_float=True),
    Entry("mpi_head_bwd", b_head_bwd, any_float=True),
    Entry("conv3x3_fwd", b_conv_fwd, absent={"bias": {}}),
    Entry("conv3x3_pack", b_conv_pack, any_float=True,
          geometry=["w_flat", "lut"]),
    Entry("conv3x3_wrw", b_wrw),
    Entry("conv3x3_wrw_bias", b_wrw),
    Entry("upsample2x_fwd", b_up_fwd, any_float=True),
    Entry("upsample2x_bwd", b_up_bwd, any_float=True),
    Entry("pack_gather", b_pack_gather, any_float=True,
          geometry=["w", "lut"]),
    Entry("conv_igemm_fwd", b_igemm_fwd, absent={"bias": {}}),
    Entry("conv_igemm_wrw", b_igemm_wrw),
    Entry("conv_igemm_wrw", b_igemm_wrw, over=DET, tag="-det"),
    Entry("eav2_fwd", b_eav2_fwd, geometry=["disp"], strided=["img"]),
    Entry("eav2_fwd", b_eav2_fwd, over={"det": True}, geometry=["disp"],
          strided=["img"], tag="-det"),
    Entry("eav2_bwd", b_eav2_bwd, geometry=["disp"], strided=["img"]),
    Entry("eav2_bwd", b_eav2_bwd, over={"det": True}, geometry=["disp"],
          strided=["img"], tag="-det"),
    Entry("gather_pxpy_bwd", b_gather, geometry=["grad_out"]),
]
IDS = [e.id for e in TABLE]


def test_table_covers_every_binding():
    ext = pytest.importorskip("mine_amd.ops._mine_hip")
    exported = {n for n in dir(ext) if not n.startswith("_")}
    assert exported == {e.binding for e in TABLE}


def _tensor_names(args):
    return [k for k, v in args.items() if isinstance(v, torch.Tensor)]


def _assert_names(err, entry, name):
    msg = str(err.value)
    # bn_act_bwd reports through the two bindings it is made of
    assert msg.startswith(entry.binding), msg
    assert f": {name} must " in msg.splitlines()[0], msg


# ---------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("entry", TABLE, ids=IDS)
def test_cpu_tensors_refused(entry):
    if torch.cuda.is_available():
        pytest.skip("the GPU part covers this machine")
    pytest.importorskip("mine_amd.ops._mine_hip")
    args = entry.args("cpu")
    with pytest.raises(RuntimeError) as err:
        entry.call(args)
    first = _tensor_names(args)[0]
    _assert_names(err, entry, first)
    assert f"{first} must be on the GPU" in str(err.value)


# ---------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------

DEV = "cuda:0"


def _wider(t, first, any_float):
    if t.dtype == F32:
        return t.to(F64)
    if t.dtype in HALVES:
        return t.to(F64 if first and any_float else F32)
    if t.dtype == I32:
        return t.to(I64)
    return None                     # int64: nothing wider


def _other16(t, first):
    if t.dtype in HALVES and not first:
        return t.to(F16 if t.dtype == BF16 else BF16)
    return None


def _noncontig(t):
    if t.numel() < 2:
        return None                 # one element is always contiguous
    big = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
    view = big[::2].view(t.shape)
    view.copy_(t)
    assert view.numel() == t.numel() and not view.is_contiguous()
    return view


def _longer(t):
    if t.dim() == 0:
        return torch.stack((t, t))
    # a flat view grows by one row of 8 channels, a shaped one by one slice
    extra = min(8, t.numel()) if t.dim() == 1 else 1
    return torch.cat((t, t.narrow(-1, 0, extra)), -1).contiguous()


def _corruptions(entry, args):
    names = _tensor_names(args)
    for name in names:
        t, first = args[name], name == names[0]
        kinds = {"wider": _wider(t, first, entry.any_float),
                 "other16": _other16(t, first),
                 "noncontig": None if name in entry.strided else _noncontig(t),
                 "longer": None if name in entry.geometry else _longer(t)}
        for kind, bad in kinds.items():
            if bad is not None:
                yield name, kind, bad


@pytest.mark.gpu
@pytest.mark.parametrize("entry", TABLE, ids=IDS)
def test_every_corruption_refused(entry):
    args = entry.args(DEV)
    entry.call(args)
    seen = set()
    for name, kind, bad in _corruptions(entry, args):
        with pytest.raises(RuntimeError) as err:
            entry.call(OrderedDict(args, **{name: bad}))
        _assert_names(err, entry, name)
        seen.add((name, kind))
    # every tensor argument met a wrong layout or size, and a wrong dtype
    # unless it is int64
    for name in _tensor_names(args):
        assert {k for n, k in seen if n == name} & {"noncontig", "longer"}
        assert (name, "wider") in seen or args[name].dtype == I64
    entry.call(args)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", [e for e in TABLE if e.absent],
                         ids=[e.id for e in TABLE if e.absent])
def test_empty_means_absent(entry):
    for name, change in entry.absent.items():
        args = entry.args(DEV)
        empty = torch.empty(0, device=DEV, dtype=args[name].dtype)
        args[name] = empty
        for k, v in change.items():
            args[k] = empty if isinstance(v, str) else v
        entry.call(args)
    torch.cuda.synchronize()


# the formerly suffixed families and upsample2x: f64 everywhere, f32 where
# only bf16 and fp16 have an instance
ANY_FLOAT = [e for e in TABLE if e.any_float and not e.id.endswith("-det")
             and e.binding not in ("conv3x3_pack", "pack_gather")]
HALF_ONLY = [e for e in TABLE if e.binding in (
    "bn_join_stats", "conv3x3_fwd", "conv3x3_wrw", "conv3x3_wrw_bias",
    "conv_igemm_fwd", "conv_igemm_wrw") and not e.id.endswith("-det")]


def _recast(args, wide):
    """Every 16-bit tensor of the call in `wide` (never narrower)."""
    return OrderedDict((k, v.to(wide) if isinstance(v, torch.Tensor)
                        and v.dtype in HALVES else v) for k, v in args.items())


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ANY_FLOAT + HALF_ONLY,
                         ids=[e.id for e in ANY_FLOAT + HALF_ONLY])
def test_f64_refused(entry):
    with pytest.raises(RuntimeError) as err:
        entry.call(_recast(entry.args(DEV), F64))
    assert "must be" in str(err.value)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ANY_FLOAT, ids=[e.id for e in ANY_FLOAT])
def test_f32_accepted_where_instantiated(entry):
    out = entry.call(_recast(entry.args(DEV), F32))
    first = out[0] if isinstance(out, (list, tuple)) else out
    assert first.dtype == F32
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", HALF_ONLY, ids=[e.id for e in HALF_ONLY])
def test_f32_refused_where_16bit_only(entry):
    with pytest.raises(RuntimeError) as err:
        entry.call(_recast(entry.args(DEV), F32))
    _assert_names(err, entry, _tensor_names(entry.args(DEV))[0])


# ---------------------------------------------------------------------------
# exact references of the two pure copies
# ---------------------------------------------------------------------------

def _nhwc_image(dtype):
    g = torch.Generator().manual_seed(11)
    n = PAD["N"] * PAD["H"] * PAD["W"] * PAD["C"]
    # distinct values that bf16 holds exactly
    x = (torch.randperm(n, generator=g) - n // 2).to(F32) * 0.5
    return x.view(PAD["N"], PAD["H"], PAD["W"], PAD["C"]).to(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_reflect_pad_fwd_exact(dtype):
    x = _nhwc_image(dtype)
    ref = F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
    ref = ref.permute(0, 2, 3, 1).contiguous().to(dtype)
    out = _ext().reflect_pad_fwd(x.reshape(-1).to(DEV), *PAD.values(), 1)
    assert out.dtype == dtype
    assert torch.equal(out.cpu().view(ref.shape), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_upsample2x_fwd_exact(dtype):
    x = _nhwc_image(dtype)
    ref = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    out = _ext().upsample2x_fwd(x.reshape(-1).to(DEV), *PAD.values())
    assert out.dtype == dtype
    assert torch.equal(out.cpu().view(ref.shape), ref)
