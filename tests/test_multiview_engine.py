"""Several target views per source image (data.num_tgt_views > 1).

The engine stages the B x L target views view-major, flattened to
(L*B, ...) with index l*B + b = view l of sample b, renders them from the
one MPI through render_tgt_views and runs every target-side loss term on
the L*B batch.
"""
import copy

import pytest
import torch

import test_collect_sim as sim
from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
from mine_amd.engine import SynthesisTask

_TGT_TERMS = ("loss_rgb_tgt", "loss_ssim_tgt", "loss_smooth_tgt",
              "loss_smooth_tgt_v2", "loss_disp_pt3dtgt", "psnr_tgt",
              "lpips_tgt")


def _items(cfg, n=2):
    ds = SyntheticMPIDataset(cfg, length=n)
    return collate_src_tgt([ds[i] for i in range(n)])


def _twice(items):
    """The same target view fed as view 0 and as view 1."""
    src, tgt = items
    return src, {k: torch.cat((v, v), dim=1) for k, v in tgt.items()}


def test_train_step_with_two_views_cpu(tiny_config):
    cfg = tiny_config.replace(**{"data.num_tgt_views": 2})
    items = _items(cfg)
    assert items[1]["img"].shape[:2] == (2, 2)
    task = SynthesisTask(cfg, device="cpu")
    loss_dict = task.train_step(items)
    for k, v in loss_dict.items():
        assert bool(torch.isfinite(v)), f"{k} = {float(v)}"
    assert float(loss_dict["loss"]) > 0
    g = task.decoder.dispconvs["0"].conv.weight.grad
    assert g is not None and g.abs().max() > 0


def test_set_data_keeps_view_major_order(tiny_config):
    cfg = tiny_config.replace(**{"data.num_tgt_views": 3})
    src, tgt = _items(cfg)
    B, L = tgt["img"].shape[:2]
    assert (B, L) == (2, 3)
    for b in range(B):
        for l in range(L):
            tgt["img"][b, l] = 10.0 * l + b       # distinguishable views
    task = SynthesisTask(cfg, device="cpu")
    task.set_data((src, tgt))
    assert task.num_tgt_views == L
    for name, key in (("tgt_imgs", "img"), ("G_src_tgt", "G_src_tgt"),
                      ("K_tgt", "K"), ("K_tgt_inv", "K_inv"),
                      ("pt3d_tgt", "xyzs")):
        staged = getattr(task, name)
        assert staged.shape == (L * B,) + tuple(tgt[key].shape[2:]), name
        for b in range(B):
            for l in range(L):
                assert torch.equal(staged[l * B + b], tgt[key][b, l].float()), \
                    f"{name}: view {l} of sample {b}"
    assert torch.equal(task.tgt_imgs[:, 0, 0, 0],
                       torch.tensor([0.0, 1.0, 10.0, 11.0, 20.0, 21.0]))
    eye = torch.matmul(task.G_tgt_src, task.G_src_tgt)
    torch.testing.assert_close(eye, torch.eye(4).expand_as(eye))


def test_duplicated_view_matches_single_view(tiny_config):
    """L = 2 with the same view twice against L = 1: the first B renders
    are the L = 1 renders bit for bit, and a mean over a duplicated batch
    differs from the mean over the batch by rounding alone."""
    items = _items(tiny_config)
    B = items[0]["img"].shape[0]
    torch.manual_seed(5)
    task = SynthesisTask(tiny_config, device="cpu")

    def run(batch):
        task.set_data(batch)
        torch.manual_seed(6)      # the stratified disparity samples
        with torch.no_grad():
            return task.loss_fcn(is_val=False)

    loss1, vis1 = run(items)
    loss2, vis2 = run(_twice(items))
    assert vis2["tgt_imgs_syn"].shape[0] == 2 * B
    assert torch.equal(vis2["tgt_imgs_syn"][:B], vis1["tgt_imgs_syn"])
    assert torch.equal(vis2["tgt_imgs_syn"][B:], vis1["tgt_imgs_syn"])
    assert torch.equal(vis2["src_imgs_syn"], vis1["src_imgs_syn"])
    for k in _TGT_TERMS:
        torch.testing.assert_close(loss2[k], loss1[k], msg=lambda m: f"{k}: {m}")
    for k in ("loss_rgb_tgt", "loss_ssim_tgt", "loss_smooth_tgt_v2",
              "loss_disp_pt3dtgt"):
        assert float(loss1[k]) != 0.0, k
    torch.testing.assert_close(loss2["loss"], loss1["loss"])


def test_static_staging_refuses_several_views(tiny_config):
    items = _twice(_items(tiny_config))
    task = SynthesisTask(tiny_config, device="cpu")
    with pytest.raises(NotImplementedError, match="one target view"):
        task.set_data(items, static=True)
    task.set_data(items)          # the eager staging takes them


# ---------------------------------------------------------------------------
# GPU: one deterministic train step with two target views, twice
# ---------------------------------------------------------------------------

def _two_view_items():
    from test_render_paths_gpu import _rodrigues
    src, tgt = sim.step_items()
    B = src["img"].shape[0]
    second = {k: v.clone() for k, v in tgt.items()}
    G = torch.eye(4)
    G[:3, :3] = _rodrigues(torch.tensor((0.02, -0.04, 0.01)))
    G[:3, 3] = torch.tensor((0.05, -0.03, 0.02))
    second["G_src_tgt"] = G.view(1, 1, 4, 4).repeat(B, 1, 1, 1)
    second["img"] = tgt["img"].flip(-1)
    return src, {k: torch.cat((tgt[k], second[k]), dim=1) for k in tgt}


@pytest.fixture
def restore_mode():
    from mine_amd.ops import backend, conv
    prev = (backend._DETERMINISTIC, conv._FORCE_IGEMM,
            torch.backends.cudnn.deterministic)
    yield
    backend._DETERMINISTIC = prev[0]
    conv.set_force_igemm(prev[1])
    torch.backends.cudnn.deterministic = prev[2]


@pytest.mark.gpu
def test_two_view_step_bit_reproducible(restore_mode):
    """test_whole_step_bit_reproducible of tests/test_deterministic_step_gpu
    with two target views per sample: the view-batched render and its
    order-fixed backward (mode 2, accumulate form of the collect pass)
    are in the step, and every loss term, gradient and updated tensor is
    bit-identical run after run."""
    from mine_amd.ops import is_deterministic
    DEV = "cuda:0"
    cfg = sim.step_config()
    items = _two_view_items()
    assert items[1]["img"].shape[1] == 2
    torch.manual_seed(61)
    task = SynthesisTask(cfg, device=DEV)
    assert is_deterministic()
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
    assert task.num_tgt_views == 2
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
    moved = [k for k in p1 if k.endswith("weight") and
             not torch.equal(p1[k], state[int(k[0])][k[2:]])]
    assert moved
