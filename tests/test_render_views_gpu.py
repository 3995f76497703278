"""The view-batched novel-view render on the GPU: V cameras, one MPI.

Forward: one launch of the single-view kernel over V*B view rows, so every
[v] slice must EQUAL render_tgt_view for that view. Backward: one grad_mpi
through one MPI-sized payload, view after view. In deterministic mode
(mode 2) the collect pass stores view 0 and adds the later views in
ascending order, so the gradient must EQUAL ((g_0 + g_1) + g_2) of the
single-view mode-2 gradients; modes 0 and 1 differ from the sum of the
single-view gradients only in the order of fp32 atomic and tile additions,
which tests/test_warp_bwd_gpu.py bounds with rtol = atol = 1e-4 for one
view (atol times V here: V such terms add).

Scenes (builders of tests/test_render_paths_gpu.py):
  A  B=2 S=5 37x45 V=3: its "odd" scene (another focal length and
     disparity list per batch element). View 0 the small random pose,
     view 1 a large translation and yaw (border-clamped pixels, and
     pixels outside: mask < S), view 2 the "cull" pose (planes of batch
     element 1 behind the camera).
  B  B=1 S=10 24x40 V=2, the "exit" sigma field: planes 1..3 opaque on
     the left half, the early exit fires, six tail planes remain.
  C  B=1 S=1 9x11 V=2.
The unmarked test asserts these properties on the CPU.
"""
import functools

import pytest
import torch

import test_render_paths_gpu as rp
from mine_amd.ops import torch_ref as tr
from mine_amd.utils.geometry import inverse_3x3

DEV = "cuda:0"
gpu = pytest.mark.gpu

_YAW = ((0.0, 0.2, 0.0), (0.3, 0.05, 0.1))
_CULL = ((0.3, 0.3, 0.0), (-0.5, 2.0, -1.6))
_SMALL = ((0.02, -0.03, 0.01), (0.04, -0.02, 0.03))


def _pose(aa, t, B):
    G = torch.eye(4)
    G[:3, :3] = rp._rodrigues(torch.tensor(aa))
    G[:3, 3] = torch.tensor(t)
    return G.unsqueeze(0).repeat(B, 1, 1)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "A":
        sc = dict(rp._build(**rp._CASES["odd"]))
        poses = [sc["G"], _pose(*_YAW, 2), _pose(*_CULL, 2)]
    elif name == "B":
        sc = dict(rp._build(B=1, S=10, H=24, W=40, seed=21,
                            disparity=[rp._EVEN_DISP],
                            sigma_fn=rp._exit_sigma))
        poses = [sc["G"], _pose(*_SMALL, 1)]
    else:
        sc = dict(rp._build(B=1, S=1, H=9, W=11, seed=2,
                            sigma_fn=rp._few_sigma))
        poses = [sc["G"], _pose(*_SMALL, 1)]
    V = len(poses)
    sc["V"] = V
    sc["Gv"] = torch.stack(poses, dim=0)                   # (V,B,4,4)
    sc["Kv"] = sc["K"].unsqueeze(0).repeat(V, 1, 1, 1)     # (V,B,3,3)
    g = torch.Generator().manual_seed(100 + sc["H"])
    sc["up_rgb"] = torch.randn(V, sc["B"], 3, sc["H"], sc["W"], generator=g)
    sc["up_depth"] = torch.randn(V, sc["B"], 1, sc["H"], sc["W"], generator=g)
    return sc


def test_scene_properties():
    a = _scene("A")
    S, H, W = a["S"], a["H"], a["W"]
    assert (a["B"], S, H, W, a["V"]) == (2, 5, 37, 45, 3)
    assert (H * W) % 256 != 0 and H * W > 256          # several blocks
    depths = torch.reciprocal(a["disparity"]).double()
    grid = tr.make_meshgrid(H, W).double()
    # view 1: clamped and outside pixels
    hinv = tr.homography_tgt_to_src(a["Gv"][1].double(), depths,
                                    a["K_inv"].double(), a["Kv"][1].double())
    p = torch.matmul(hinv.reshape(-1, 3, 3), grid.reshape(3, -1))
    u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
    clamped = (u < 0) | (u > W - 1) | (v < 0) | (v > H - 1)
    outside = (u <= -1) | (u >= W) | (v <= -1) | (v >= H)
    print(f"view 1: clamped share {clamped.double().mean():.3f}, outside "
          f"share {outside.double().mean():.3f}")
    assert 0.1 < clamped.double().mean() < 0.9
    assert outside.any() and not outside.all()
    # view 2: whole planes of batch element 1 behind the camera
    xyz = tr.tgt_plane_xyz(
        tr.src_plane_xyz(grid.float(), a["disparity"], a["K_inv"]),
        a["Gv"][2])
    behind = (xyz[1, :, 2] < 0).flatten(1).all(dim=1)
    print("view 2: planes of batch element 1 behind the camera:",
          behind.tolist())
    assert behind.any() and not behind.all()
    b = _scene("B")
    assert (b["B"], b["S"], b["H"], b["W"], b["V"]) == (1, 10, 24, 40, 2)
    assert float(b["sigma"][0, 1, 0, 0, 0]) > 30.0 and \
        float(b["sigma"][0, 1, 0, 0, -1]) <= 0.05
    c = _scene("C")
    assert (c["B"], c["S"], c["H"], c["W"], c["V"]) == (1, 1, 9, 11, 2)
    for sc in (a, b, c):
        assert not torch.equal(sc["Gv"][0], sc["Gv"][1])


def _ext():
    from mine_amd.ops.backend import get_extension
    return get_extension(required=True)


@pytest.fixture
def restore_mode():
    from mine_amd.ops import backend
    prev = (backend._DETERMINISTIC, torch.backends.cudnn.deterministic)
    yield
    backend._DETERMINISTIC = prev[0]
    torch.backends.cudnn.deterministic = prev[1]


def _mpi(sc, alpha):
    from mine_amd.ops.renderer import pack_mpi
    sigma = rp._alpha_of(sc["sigma"]) if alpha else sc["sigma"]
    return pack_mpi(sc["rgb"], sigma).to(DEV)


def _views(sc, mpi, bg_inf=False, alpha=False):
    from mine_amd.ops import render_tgt_views
    return render_tgt_views(mpi, sc["disparity"].to(DEV), sc["Gv"].to(DEV),
                            sc["K_inv"].to(DEV), sc["Kv"].to(DEV),
                            bg_depth_inf=bg_inf, use_alpha=alpha)


def _single(sc, mpi, v, bg_inf=False, alpha=False):
    from mine_amd.ops import render_tgt_view
    return render_tgt_view(mpi, sc["disparity"].to(DEV), sc["Gv"][v].to(DEV),
                           sc["K_inv"].to(DEV), sc["Kv"][v].to(DEV),
                           bg_depth_inf=bg_inf, use_alpha=alpha)


def _grad_views(sc, bg_inf, up_rgb=True, up_depth=True):
    mpi = _mpi(sc, False).requires_grad_(True)
    rgb, depth, _ = _views(sc, mpi, bg_inf)
    loss = 0.0
    if up_rgb:
        loss = loss + (rgb * sc["up_rgb"].to(DEV)).sum()
    if up_depth:
        loss = loss + (depth * sc["up_depth"].to(DEV)).sum()
    loss.backward()
    return mpi.grad


def _grad_single(sc, v, bg_inf, up_rgb=True, up_depth=True):
    mpi = _mpi(sc, False).requires_grad_(True)
    rgb, depth, _ = _single(sc, mpi, v, bg_inf)
    loss = 0.0
    if up_rgb:
        loss = loss + (rgb * sc["up_rgb"][v].to(DEV)).sum()
    if up_depth:
        loss = loss + (depth * sc["up_depth"][v].to(DEV)).sum()
    loss.backward()
    return mpi.grad


def _left_to_right(sc, bg_inf, **kw):
    total = _grad_single(sc, 0, bg_inf, **kw)
    for v in range(1, sc["V"]):
        total = total + _grad_single(sc, v, bg_inf, **kw)
    return total


# ---------------------------------------------------------------------------
# 1. forward, exact
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", ["plain", "bg_inf", "alpha"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_equals_single_view(name, mode):
    sc = _scene(name)
    bg_inf, alpha = mode == "bg_inf", mode == "alpha"
    with torch.no_grad():
        mpi = _mpi(sc, alpha)
        out = _views(sc, mpi, bg_inf, alpha)
        V, B, H, W = sc["V"], sc["B"], sc["H"], sc["W"]
        assert [tuple(o.shape) for o in out] == [(V, B, c, H, W)
                                                 for c in (3, 1, 1)]
        for v in range(V):
            one = _single(sc, mpi, v, bg_inf, alpha)
            for label, a, b in zip(("rgb", "depth", "mask"), out, one):
                bad = (a[v] != b).sum().item()
                assert torch.equal(a[v], b), \
                    f"{name} {mode} view {v} {label}: {bad} entries differ"
        assert bool(torch.isfinite(out[0]).all())
        assert not torch.equal(out[0][0], out[0][1])
    if name == "A":
        assert float(out[2][1].min()) < sc["S"]        # pixels outside


# ---------------------------------------------------------------------------
# 2. backward mode 2, exact and repeatable
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("bg_inf", [False, True])
@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_mode2_is_the_left_to_right_sum(name, bg_inf, restore_mode):
    from mine_amd.ops import deterministic
    sc = _scene(name)
    with deterministic():
        got = _grad_views(sc, bg_inf)
        again = _grad_views(sc, bg_inf)
        want = _left_to_right(sc, bg_inf)
    assert bool(torch.isfinite(got).all()) and got.abs().max() > 0
    bad = (got != want).sum().item()
    print(f"{name} bg_inf={int(bg_inf)}: {bad} of {got.numel()} entries "
          f"differ, max |diff| = {(got - want).abs().max().item():.3e}")
    assert torch.equal(got, want)
    assert torch.equal(again, got)


# ---------------------------------------------------------------------------
# 3. backward modes 0 and 1
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", [0, 1])
def test_backward_atomic_modes_match_the_sum(mode, monkeypatch, restore_mode):
    from mine_amd.ops import deterministic, renderer
    if mode == 0:
        monkeypatch.setenv("MINE_TGT_BWD", "scatter")
    else:
        monkeypatch.delenv("MINE_TGT_BWD", raising=False)
    monkeypatch.setattr(renderer, "_TGT_BWD_MODE", None)
    sc = _scene("A")
    with deterministic(False):
        assert renderer.tgt_bwd_mode() == mode
        got = _grad_views(sc, False)
        ref = sum(_grad_single(sc, v, False).double() for v in range(sc["V"]))
    err = (got.double() - ref).abs()
    bound = sc["V"] * 1e-4 + 1e-4 * ref.abs()
    print(f"mode {mode}: worst err/bound = {(err / bound).max().item():.3g}, "
          f"max err = {err.max().item():.3e}, max |ref| = "
          f"{ref.abs().max().item():.3e}")
    torch.testing.assert_close(got.double(), ref, rtol=1e-4,
                               atol=sc["V"] * 1e-4)


# ---------------------------------------------------------------------------
# bindings: empty upstream gradients, workspace, refusals
# ---------------------------------------------------------------------------

def _binding_args(sc, bg_inf=False):
    """The argument list of tgt_views_bwd as render_tgt_views builds it."""
    V, B, S = sc["V"], sc["B"], sc["S"]
    to = lambda t: t.contiguous().to(DEV)
    # on the device, as the op does: the same bits
    depths = torch.reciprocal(to(sc["disparity"]))
    G = to(sc["Gv"]).reshape(V * B, 4, 4)
    K_si = to(sc["K_inv"]).repeat(V, 1, 1)
    hinv = tr.homography_tgt_to_src(G, depths.repeat(V, 1), K_si,
                                    to(sc["Kv"]).reshape(V * B, 3, 3))
    hfwd = inverse_3x3(hinv.reshape(-1, 3, 3))
    return dict(mpi=_mpi(sc, False), hinv=to(hinv.reshape(V, B, S, 3, 3)),
                hfwd=to(hfwd.reshape(V, B, S, 3, 3)),
                m=to(torch.matmul(G[:, :3, :3], K_si).reshape(V, B, 3, 3)),
                tvec=to(G[:, :3, 3].reshape(V, B, 3)), depths=to(depths),
                views=V, bg_inf=bg_inf, alpha=False,
                g_rgb=to(sc["up_rgb"]), g_depth=to(sc["up_depth"]), mode=2)


def _bwd(args, **over):
    a = dict(args)
    a.update(over)
    return _ext()._views.tgt_views_bwd(**a)


@gpu
@pytest.mark.parametrize("bg_inf", [False, True])
def test_empty_upstream_gradient_is_a_zero_one(bg_inf, restore_mode):
    from mine_amd.ops import deterministic
    sc = _scene("A")
    args = _binding_args(sc, bg_inf)
    empty = torch.empty(0, device=DEV)
    full = _bwd(args)
    for absent, kw in (("g_depth", dict(up_depth=False)),
                       ("g_rgb", dict(up_rgb=False))):
        zeroed = _bwd(args, **{absent: torch.zeros_like(args[absent])})
        got = _bwd(args, **{absent: empty})
        assert got.abs().max() > 0
        assert torch.equal(got, zeroed), absent
        assert not torch.equal(got, full), absent
        # and through the op: a loss on the other output alone
        with deterministic():
            op = _grad_views(sc, bg_inf, **kw)
            want = _left_to_right(sc, bg_inf, **kw)
        assert torch.equal(op, want), absent
        assert torch.equal(op, zeroed), absent


@gpu
def test_workspace_contents_do_not_matter(restore_mode):
    sc = _scene("A")
    args = _binding_args(sc)
    own = _bwd(args)
    ws = torch.full_like(args["mpi"], float("nan"))
    got = _bwd(args, workspace=ws)
    assert bool(torch.isfinite(got).all())
    assert bool(torch.isfinite(ws).all())      # every entry was written
    assert torch.equal(got, own)
    for mode in (0, 1):
        g = _bwd(args, mode=mode,
                 workspace=torch.full_like(args["mpi"], float("nan")))
        torch.testing.assert_close(g, own, rtol=1e-4, atol=sc["V"] * 1e-4)


def _fwd_args(sc):
    a = _binding_args(sc)
    return {k: a[k] for k in ("mpi", "hinv", "m", "tvec", "depths", "views",
                              "bg_inf", "alpha")}


def _refusals(args):
    """(label, changed arguments, text the message must hold)"""
    V, B, S = args["views"], args["mpi"].shape[0], args["mpi"].shape[1]
    H, W = args["mpi"].shape[2:4]
    wide = torch.zeros(args["m"].shape[:-1] + (6,), device=DEV)[..., ::2]
    assert wide.shape == args["m"].shape and not wide.is_contiguous()
    S193 = 193
    return [
        ("short hinv",
         dict(hinv=args["hinv"].flatten()[:V * B * S * 9 - 9].clone()),
         f"hinv must have {V * B * S * 9} elements"),
        ("non-contiguous m", dict(m=wide), "m must be contiguous"),
        ("f16 mpi", dict(mpi=args["mpi"].half()), "mpi must be f32"),
        ("S = 193",
         dict(mpi=torch.zeros(B, S193, 2, 2, 4, device=DEV),
              hinv=torch.zeros(V, B, S193, 3, 3, device=DEV),
              depths=torch.ones(B, S193, device=DEV)),
         "S too large"),
        ("V = 0",
         dict(views=0, hinv=torch.zeros(0, B, S, 3, 3, device=DEV),
              m=torch.zeros(0, B, 3, 3, device=DEV),
              tvec=torch.zeros(0, B, 3, device=DEV)),
         "views must be at least 1"),
        ("depths of another batch size",
         dict(depths=torch.ones(B + 1, S, device=DEV)),
         f"depths must have {B * S} elements"),
        ("too many view rows",
         dict(views=65535), "too large for the grid"),
    ]


@gpu
@pytest.mark.parametrize("binding", ["tgt_views_fwd", "tgt_views_bwd"])
def test_binding_refusals(binding):
    sc = _scene("A")
    args = _fwd_args(sc) if binding == "tgt_views_fwd" else _binding_args(sc)
    fn = getattr(_ext()._views, binding)
    fn(**args)                                  # the unchanged call runs
    cases = _refusals(args)
    if binding == "tgt_views_bwd":
        cases += [
            ("short hfwd", dict(hfwd=args["hfwd"][:1].clone()),
             "hfwd must have"),
            ("g_rgb of one view", dict(g_rgb=args["g_rgb"][0].clone()),
             "g_rgb must have"),
            ("unknown mode", dict(mode=3), "unknown mode"),
            ("small workspace",
             dict(workspace=torch.zeros(4, device=DEV)),
             "workspace must have"),
        ]
    for label, change, text in cases:
        bad = dict(args)
        bad.update(change)
        with pytest.raises(RuntimeError) as err:
            fn(**bad)
        msg = str(err.value).splitlines()[0]
        assert msg.startswith(binding + ": "), (label, msg)
        assert text in msg, (label, msg)


def test_cpu_tensors_refused():
    ext = _ext()       # a missing extension is an error, not a skip
    z = torch.zeros
    with pytest.raises(RuntimeError, match="^tgt_views_fwd: mpi must be on "
                                           "the GPU"):
        ext._views.tgt_views_fwd(z(1, 1, 2, 2, 4), z(1, 1, 1, 3, 3),
                                 z(1, 1, 3, 3), z(1, 1, 3), z(1, 1), 1,
                                 False, False)
    with pytest.raises(RuntimeError, match="^tgt_views_bwd: mpi must be on "
                                           "the GPU"):
        ext._views.tgt_views_bwd(z(1, 1, 2, 2, 4), z(1, 1, 1, 3, 3),
                                 z(1, 1, 1, 3, 3), z(1, 1, 3, 3), z(1, 1, 3),
                                 z(1, 1), 1, False, False, z(0), z(0), 2)
