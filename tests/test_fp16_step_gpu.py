"""Whole train steps with training.amp_dtype: fp16 on the config of
test_gpu_ops.py::test_full_train_step_gpu, and bit-reproducible network
gradients in fp16 under training.deterministic (as
test_deterministic_gpu.py::test_network_bit_reproducible asserts for
bf16).

The GradScaler's starting scale. torch's default, 2^16, is too high for
this network: measured on an MI355X with this config, step 1 at 2^16
overflows almost every gradient, step 2 at 2^15 still overflows a few
elements of the stem's and the coarsest dispconv's weight gradients, and
step 3 at 2^14 has its largest fp16 weight gradient at 6.43e4 against the
fp16 limit 65504 -- so whether one of three steps is applied depends on
the order of the fp32 atomics (seen both ways in two runs of the same
code; the commit before the fp16 kernels behaves the same way, its third
step at 2^14 still overflowed 5 elements). Those gradients come from the
two convolutions that still run in the library with an fp16 copy of the
weight (docs/NEXT.md section 7, weight routing), not from the kernels
under test. The test therefore starts the scaler at 2^12, a factor 4 below
the borderline, which makes the outcome independent of that noise, and
asks for more than one applied step: none of the three may be skipped."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture
def restore_mode():
    from mine_amd.ops import backend, conv
    prev = (backend._DETERMINISTIC, conv._FORCE_IGEMM,
            torch.backends.cudnn.deterministic)
    yield
    backend._DETERMINISTIC = prev[0]
    conv.set_force_igemm(prev[1])
    torch.backends.cudnn.deterministic = prev[2]


def _same_bits(a, b):
    """Bit identity, NaN payloads included."""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def test_fp16_train_steps():
    from mine_amd.config import default_config
    from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
    from mine_amd.engine import SynthesisTask

    cfg = default_config(**{
        "data.name": "realestate10k", "data.img_h": 128, "data.img_w": 192,
        "mpi.num_bins_coarse": 32, "data.per_gpu_batch_size": 2,
        "data.visible_point_count": 64,
        "lr.decay_steps": [4, 8],
        "training.amp_dtype": "fp16",
    })
    ds = SyntheticMPIDataset(cfg, length=2)
    items = collate_src_tgt([ds[0], ds[1]])
    torch.manual_seed(71)
    task = SynthesisTask(cfg, device=DEV)
    assert task.amp_dtype == torch.float16 and task.grad_scaler is not None
    init_scale = 2.0 ** 12    # see the module docstring
    task.grad_scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    nets = [task.backbone, task.decoder]
    before = [p.detach().clone() for n in nets for p in n.parameters()]
    for _ in range(3):
        loss_dict = task.train_step(items)
    loss = float(loss_dict["loss"])
    scale = float(task.grad_scaler.get_scale())
    print(f"loss {loss:.4f}, GradScaler scale {scale}")
    assert loss == loss and abs(loss) < 1e6
    assert scale > 0
    assert scale == init_scale    # a skipped step would have halved it
    after = [p.detach() for n in nets for p in n.parameters()]
    # the steps were applied: parameters moved and stayed finite
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    assert all(torch.isfinite(a).all() for a in after)


def test_fp16_network_bit_reproducible(restore_mode):
    from mine_amd.config import default_config
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import is_deterministic

    B, S, H, W = 2, 8, 128, 192
    cfg = default_config(**{
        "data.name": "synthetic", "data.img_h": H, "data.img_w": W,
        "mpi.num_bins_coarse": S, "data.per_gpu_batch_size": B,
        "data.visible_point_count": 32, "data.num_workers": 0,
        "training.deterministic": True,
        "training.amp_dtype": "fp16",
    })
    torch.manual_seed(61)
    task = SynthesisTask(cfg, device=DEV)
    assert is_deterministic()
    assert task.amp_dtype == torch.float16 and task.channels_last
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
        if ups is None:
            ups = [torch.randn(o.shape, generator=g).to(DEV) for o in outs]
        torch.autograd.backward(outs, ups)
        grads = {f"{i}.{k}": p.grad.detach().clone()
                 for i, n in enumerate(nets)
                 for k, p in n.named_parameters() if p.grad is not None}
        return [o.detach().clone() for o in outs], grads

    outs1, grads1 = run()
    outs2, grads2 = run()
    for s, (a, b) in enumerate(zip(outs1, outs2)):
        assert _same_bits(a, b), f"MPI scale {s} differs"
    assert grads1 and grads1.keys() == grads2.keys()
    assert any(g.abs().sum() > 0 for g in grads1.values())
    bad = [k for k in grads1 if not _same_bits(grads1[k], grads2[k])]
    assert not bad, f"{len(bad)} of {len(grads1)} gradients differ: {bad[:8]}"
