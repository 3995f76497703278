"""render_tgt_views on the CPU path: V cameras, one MPI.

The CPU path loops `torch_ref.render_tgt_reference` over the views, so
the outputs equal the stacked single-view renders exactly, and the MPI
gradient is the sum of the per-view gradients (autograd chooses the
order of that sum, hence assert_close defaults).
"""
import pytest
import torch

import test_render_paths_gpu as rp
from mine_amd.ops import render_tgt_view, render_tgt_views
from mine_amd.ops.renderer import pack_mpi

V = 3


def _case():
    sc = rp._build(B=2, S=4, H=13, W=17, seed=11, focal=(0.8, 1.1))
    g = torch.Generator().manual_seed(12)
    G = sc["G"].unsqueeze(0).repeat(V, 1, 1, 1)
    G[1:, :, :3, 3] += 0.1 * torch.randn(V - 1, sc["B"], 3, generator=g)
    K_tgt = sc["K"].unsqueeze(0).repeat(V, 1, 1, 1)
    K_tgt[2, :, 0, 0] *= 1.2       # another focal length in the last view
    up = [torch.randn(V, sc["B"], c, sc["H"], sc["W"], generator=g)
          for c in (3, 1)]
    return sc, G, K_tgt, up


@pytest.mark.parametrize("bg_inf,alpha", [(False, False), (True, False),
                                          (False, True)])
def test_cpu_views_equal_stacked_single_views(bg_inf, alpha):
    sc, G, K_tgt, _ = _case()
    mpi = pack_mpi(sc["rgb"], sc["sigma"] * (0.3 if alpha else 1.0))
    out = render_tgt_views(mpi, sc["disparity"], G, sc["K_inv"], K_tgt,
                           bg_depth_inf=bg_inf, use_alpha=alpha)
    assert [tuple(o.shape) for o in out] == [
        (V, sc["B"], c, sc["H"], sc["W"]) for c in (3, 1, 1)]
    for v in range(V):
        one = render_tgt_view(mpi, sc["disparity"], G[v], sc["K_inv"],
                              K_tgt[v], bg_depth_inf=bg_inf, use_alpha=alpha)
        for name, a, b in zip(("rgb", "depth", "mask"), out, one):
            assert torch.equal(a[v], b), f"view {v}: {name}"
    # the views are different pictures
    assert not torch.equal(out[0][0], out[0][1])


def test_cpu_views_gradient_is_the_sum_over_views():
    sc, G, K_tgt, (up_rgb, up_depth) = _case()

    def grad(fn):
        mpi = pack_mpi(sc["rgb"], sc["sigma"]).requires_grad_(True)
        fn(mpi).backward()
        return mpi.grad

    def batched(mpi):
        rgb, depth, _ = render_tgt_views(mpi, sc["disparity"], G,
                                         sc["K_inv"], K_tgt)
        return (rgb * up_rgb).sum() + (depth * up_depth).sum()

    def single(v):
        def fn(mpi):
            rgb, depth, _ = render_tgt_view(mpi, sc["disparity"], G[v],
                                            sc["K_inv"], K_tgt[v])
            return (rgb * up_rgb[v]).sum() + (depth * up_depth[v]).sum()
        return fn

    got = grad(batched)
    want = sum(grad(single(v)) for v in range(V))
    assert got.shape == (sc["B"], sc["S"], sc["H"], sc["W"], 4)
    assert want.abs().max() > 0
    torch.testing.assert_close(got, want)


def test_views_shape_mismatch_is_refused():
    sc, G, K_tgt, _ = _case()
    mpi = pack_mpi(sc["rgb"], sc["sigma"])
    with pytest.raises(ValueError, match="render_tgt_views"):
        render_tgt_views(mpi, sc["disparity"], G[:, :1], sc["K_inv"], K_tgt)
    with pytest.raises(ValueError, match="render_tgt_views"):
        render_tgt_views(mpi, sc["disparity"], G[0], sc["K_inv"], K_tgt[0])
