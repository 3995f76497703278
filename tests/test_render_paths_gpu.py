"""Renderer kernels on the paths the first-round tests never reach.

Every comparison is HIP kernel (fp32) against the project's own eager
path (`render_src_view` / `render_tgt_view` on CPU tensors, i.e.
`torch_ref`) run in fp64. Four scenes:

  odd    B=2 S=5 37x45: HW=1665 (partial last block of 256), 2x2 gather
         tiles with partial edge tiles, a different focal length and a
         different disparity list per batch element. Batch element 1
         carries one plane behind the target camera (disparity 12), so
         the gather kernel's whole-image bbox fallback and the z-cull
         are reached at this shape too.
  few    S=1 and S=2 at 9x11.
  exit   S=10 24x40, left half opaque on planes 1..3 (sigma*delta >= 36):
         each opaque plane multiplies the transmittance by ~1e-6 (the
         +1e-6 of the reference), so A < 1e-14 after plane 3 and six tail
         planes remain for the copy-through / pass-through / mask tails.
  cull   S=8 24x40, target camera moved forward by 1.6, yawed and pitched
         0.3 rad each and offset by (-0.5, 2.0): three planes lie behind it
         and the plane at depth 2 has both signs of z inside the image.
         Forward motion and yaw alone cannot give that with a finite
         homography: the ray/plane intersection has one sign per plane
         unless the plane's horizon crosses the image, where hz -> 0. The
         mixed plane comes from the border clamp instead: with the pitch
         the z = 0 line runs diagonally through the source image, and
         target pixels that land above its top border are clamped onto
         the far side of that line.

The unmarked tests run on the CPU and assert that the scenes really
have these properties (dead shares, z signs, bbox fallback taken and
not taken, excluded share under 1 %).

Exclusions: the oracle decides u > -1, u < W, the border clamp and
z >= 0 in fp64, the kernel in fp32. Target pixels where the fp64 oracle
has |z| < 1e-4 or u/v within 1e-3 of one of those boundaries, for any
plane, are left out of the forward comparison and get a zero upstream
gradient (on both sides) in the backward comparison.

Tolerances are the ones tests/test_gpu_ops.py applies to the same
outputs. For the tgt backward with bg_inf the atol is multiplied by
r = median|oracle grad_sigma, bg_inf| / median|oracle grad_sigma, not
bg_inf| (both fp64, same scene and upstream gradients, floored at 1; 1
when more than half of the entries are exactly zero): the bg-inf depth
term puts |e| ~ 1e3 into the sigma gradient.
"""
import functools

import pytest
import torch

from mine_amd.ops import torch_ref as tr
from mine_amd.utils.geometry import inverse_3x3

DEV = "cuda:0"
GT = 32          # gather tile side of tgt_gather_kernel
DEAD = 1e-14     # early-exit threshold of the kernels


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------

def _rodrigues(aa):
    th = aa.norm()
    k = aa / (th + 1e-9)
    Kx = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return torch.eye(3) + th.sin() * Kx + (1 - th.cos()) * (Kx @ Kx)


def _build(B, S, H, W, seed, focal=(0.8,), disparity=None, pose=None,
           sigma_fn=None):
    """fp32 CPU scene. focal: per-batch multiples of W (cycled);
    disparity: (B,S) list or None for sorted random; pose: per-batch
    (axis-angle, translation) or None for the small random pose of the
    first-round scenes; sigma_fn(sigma, depths) -> sigma edits the field."""
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(B, S, 3, H, W, generator=g)
    sigma = torch.rand(B, S, 1, H, W, generator=g) * 3.0 + 1e-4
    rand_disp, _ = torch.sort(torch.rand(B, S, generator=g) * 0.95 + 0.02,
                              dim=1, descending=True)
    if disparity is None:
        disparity = rand_disp
    else:
        disparity = torch.tensor(disparity, dtype=torch.float32)
        assert disparity.shape == (B, S)
    K = torch.zeros(B, 3, 3)
    for b in range(B):
        f = focal[b % len(focal)] * W
        K[b] = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2],
                             [0.0, 0.0, 1.0]])
    K_inv = torch.inverse(K)
    aa = 0.05 * torch.randn(B, 3, generator=g)
    G = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
    for b in range(B):
        if pose is None:
            G[b, :3, :3] = _rodrigues(aa[b])
            G[b, :3, 3] = 0.15 * torch.randn(3, generator=g)
        else:
            G[b, :3, :3] = _rodrigues(torch.tensor(pose[b][0]))
            G[b, :3, 3] = torch.tensor(pose[b][1])
    img = torch.rand(B, 3, H, W, generator=g)
    if sigma_fn is not None:
        sigma = sigma_fn(sigma, torch.reciprocal(disparity), g)
    # upstream gradients
    wr = torch.randn(B, 3, H, W, generator=g)
    wd = torch.randn(B, 1, H, W, generator=g)
    wb = torch.randn(B, S, H, W, 4, generator=g)
    return dict(rgb=rgb, sigma=sigma, disparity=disparity, K=K, K_inv=K_inv,
                G=G, img=img, wr=wr, wd=wd, wb=wb, B=B, S=S, H=H, W=W)


_EXIT_PLANES = (1, 2, 3)


def _exit_sigma(sigma, depths, g):
    """Left half: planes 1..3 opaque with sigma*(d_{s+1}-d_s) = 36, so
    sigma*delta >= 36 in both views (a segment between two parallel
    planes is at least as long as their distance) and t = exp(-36) is far
    below the 1e-6 that the reference adds. Not more than that: where the
    warp interpolates across the opaque edge, an fp32 rounding of u moves
    the sampled sigma by sigma_opaque * 1e-6 and with it the gradient.
    Right half: sigma <= 0.05 on every plane."""
    B, S, _, H, W = sigma.shape
    out = 0.05 * torch.rand(B, S, 1, H, W, generator=g)
    for s in _EXIT_PLANES:
        gap = (depths[:, s + 1] - depths[:, s]).view(B, 1, 1, 1)
        out[:, s, :, :, :W // 2] = 36.0 / gap
    return out


def _few_sigma(sigma, depths, g):
    """Thin media, so that with one or two planes the sigma gradient is
    not exp(-sigma*1e3) ~ 0 on the far plane: sigma*1e3 <= 3 there and
    sigma <= 0.3 on the plane in front of it."""
    out = sigma * 0.1
    out[:, -1] = sigma[:, -1] * 1e-3
    return out


_EVEN_DISP = [0.95 - 0.1 * i for i in range(10)]
_CULL_DISP = [0.9, 0.8, 0.7, 0.5, 0.3, 0.2, 0.1, 0.05]

_CASES = {
    # seed 6 draws t_z = -0.132 for batch element 1, so its nearest plane
    # (depth 1/12) lies behind the target camera: z = -0.05 everywhere
    "odd": dict(B=2, S=5, H=37, W=45, seed=6, focal=(0.8, 1.1),
                disparity=[[0.93, 0.61, 0.37, 0.18, 0.04],
                           [12.0, 0.77, 0.52, 0.29, 0.07]]),
    "few1": dict(B=2, S=1, H=9, W=11, seed=2, focal=(0.8, 1.1),
                 sigma_fn=_few_sigma),
    "few2": dict(B=2, S=2, H=9, W=11, seed=3, focal=(0.8, 1.1),
                 sigma_fn=_few_sigma),
    "exit": dict(B=2, S=10, H=24, W=40, seed=21,
                 disparity=[_EVEN_DISP, _EVEN_DISP], sigma_fn=_exit_sigma),
    "cull": dict(B=1, S=8, H=24, W=40, seed=6, disparity=[_CULL_DISP],
                 pose=[((0.3, 0.3, 0.0), (-0.5, 2.0, -1.6))]),
}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _build(**_CASES[name])


# ---------------------------------------------------------------------------
# fp64 geometry of the warp: exclusions, z signs, bbox replay
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _geometry(name):
    """u, v, z, hz of every (b, s, tgt pixel) in fp64, as the oracle sees
    them: (u, v) = perspective divide of H_src_tgt p, z = third row of
    R K^-1 (clamped u, v, 1) d + t."""
    sc = _scene(name)
    B, S, H, W = sc["B"], sc["S"], sc["H"], sc["W"]
    d64 = lambda t: t.double()
    depths = torch.reciprocal(d64(sc["disparity"]))
    hinv = tr.homography_tgt_to_src(d64(sc["G"]), depths, d64(sc["K_inv"]),
                                    d64(sc["K"]))
    grid = tr.make_meshgrid(H, W).double().reshape(3, -1)
    mapped = torch.matmul(hinv, grid).reshape(B, S, 3, H, W)
    hz = mapped[:, :, 2]
    u = mapped[:, :, 0] / hz
    v = mapped[:, :, 1] / hz
    ucl = u.clamp(0, W - 1)
    vcl = v.clamp(0, H - 1)
    M = torch.matmul(d64(sc["G"])[:, :3, :3], d64(sc["K_inv"]))
    row = M[:, 2].view(B, 1, 3, 1, 1)
    z = (row[:, :, 0] * ucl + row[:, :, 1] * vcl + row[:, :, 2]) \
        * depths.view(B, S, 1, 1) + d64(sc["G"])[:, 2, 3].view(B, 1, 1, 1)
    return u, v, z, hz


@functools.lru_cache(maxsize=None)
def _keep(name):
    """(B,H,W) bool: target pixels that take part in the comparison."""
    sc = _scene(name)
    H, W = sc["H"], sc["W"]
    u, v, z, _ = _geometry(name)
    bad = z.abs() < 1e-4
    for edge in (-1.0, 0.0, W - 1.0, float(W)):
        bad |= (u - edge).abs() < 1e-3
    for edge in (-1.0, 0.0, H - 1.0, float(H)):
        bad |= (v - edge).abs() < 1e-3
    bad |= ~(torch.isfinite(u) & torch.isfinite(v))
    return ~bad.any(dim=1)


def _fallback_tiles(name):
    """Replay the bbox rule of tgt_gather_kernel in fp32: True where the
    (b, s, tile) takes the whole-image fallback."""
    sc = _scene(name)
    B, S, H, W = sc["B"], sc["S"], sc["H"], sc["W"]
    depths = torch.reciprocal(sc["disparity"]).float()
    hinv = tr.homography_tgt_to_src(sc["G"], depths, sc["K_inv"], sc["K"])
    hf = inverse_3x3(hinv.reshape(B * S, 3, 3)).reshape(B, S, 3, 3)
    tiles_x, tiles_y = (W + GT - 1) // GT, (H + GT - 1) // GT
    out = torch.zeros(B, S, tiles_y * tiles_x, dtype=torch.bool)
    for t in range(tiles_x * tiles_y):
        tx0, ty0 = (t % tiles_x) * GT, (t // tiles_x) * GT
        ok = torch.ones(B, S, dtype=torch.bool)
        for x in (tx0 - 1.25, tx0 + GT + 0.25):
            for y in (ty0 - 1.25, ty0 + GT + 0.25):
                qz = hf[..., 2, 0] * x + hf[..., 2, 1] * y + hf[..., 2, 2]
                qx = (hf[..., 0, 0] * x + hf[..., 0, 1] * y + hf[..., 0, 2]) / qz
                qy = (hf[..., 1, 0] * x + hf[..., 1, 1] * y + hf[..., 1, 2]) / qz
                ok &= (qz > 1e-8) & torch.isfinite(qx) & torch.isfinite(qy)
        out[:, :, t] = ~ok
    return out


# ---------------------------------------------------------------------------
# the two sides
# ---------------------------------------------------------------------------

def _alpha_of(sigma):
    return sigma / 3.2  # sigma in (0, 3.0001] -> alpha in (0, 0.94)


def _run_src(name, device, dtype, blend, bg_inf):
    from mine_amd.ops.renderer import pack_mpi, render_src_view
    sc = _scene(name)
    cast = lambda t: t.detach().clone().to(device=device, dtype=dtype)
    r = cast(sc["rgb"]).requires_grad_(True)
    s = cast(sc["sigma"]).requires_grad_(True)
    rgb_s, depth_s, blend_s = render_src_view(
        pack_mpi(r, s), cast(sc["disparity"]), cast(sc["K_inv"]),
        src_img=cast(sc["img"]) if blend else None, bg_depth_inf=bg_inf)
    loss = (rgb_s * cast(sc["wr"])).sum() + (depth_s * cast(sc["wd"])).sum()
    if blend:
        loss = loss + (blend_s * cast(sc["wb"])).sum()
    loss.backward()
    out = dict(rgb=rgb_s, depth=depth_s, grad_rgb=r.grad, grad_sigma=s.grad)
    if blend:
        out["blend"] = blend_s
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _run_tgt(name, device, dtype, bg_inf, alpha):
    from mine_amd.ops.renderer import pack_mpi, render_tgt_view
    sc = _scene(name)
    keep = _keep(name).unsqueeze(1)
    cast = lambda t: t.detach().clone().to(device=device, dtype=dtype)
    r = cast(sc["rgb"]).requires_grad_(True)
    s = cast(_alpha_of(sc["sigma"]) if alpha else sc["sigma"]) \
        .requires_grad_(True)
    o_rgb, o_depth, o_mask = render_tgt_view(
        pack_mpi(r, s), cast(sc["disparity"]), cast(sc["G"]),
        cast(sc["K_inv"]), cast(sc["K"]), bg_depth_inf=bg_inf,
        use_alpha=alpha)
    loss = (o_rgb * cast(sc["wr"] * keep)).sum() + \
        (o_depth * cast(sc["wd"] * keep)).sum()
    loss.backward()
    out = dict(rgb=o_rgb, depth=o_depth, mask=o_mask, grad_rgb=r.grad,
               grad_sigma=s.grad)
    return {k: v.detach().double().cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _oracle_src(name, blend, bg_inf):
    return _run_src(name, "cpu", torch.float64, blend, bg_inf)


@functools.lru_cache(maxsize=None)
def _oracle_tgt(name, bg_inf, alpha):
    return _run_tgt(name, "cpu", torch.float64, bg_inf, alpha)


def _bg_inf_ratio(name, alpha):
    """r of the module docstring, from the fp64 oracle alone."""
    a = _oracle_tgt(name, True, alpha)["grad_sigma"].abs().median().item()
    b = _oracle_tgt(name, False, alpha)["grad_sigma"].abs().median().item()
    return max(1.0, a / b) if b > 0.0 else 1.0


def _check(label, got, ref, rtol, atol, keep=None):
    """assert_close's rule |got - ref| <= atol + rtol*|ref|, printing the
    worst err/bound ratio first."""
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    ratio = (got - ref).abs() / (atol + rtol * ref.abs())
    if keep is not None:
        ratio = torch.where(keep.expand_as(ratio), ratio,
                            torch.zeros_like(ratio))
    worst = ratio.max().item()
    print(f"{label}: worst err/bound = {worst:.3g}")
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output"
    assert worst <= 1.0, f"{label}: err/bound = {worst:.4g}"


def _check_src(name, blend, bg_inf):
    got = _run_src(name, DEV, torch.float32, blend, bg_inf)
    ref = _oracle_src(name, blend, bg_inf)
    tag = f"src[{name} blend={int(blend)} bg_inf={int(bg_inf)}]"
    _check(tag + " rgb", got["rgb"], ref["rgb"], 1e-4, 1e-5)
    _check(tag + " depth", got["depth"], ref["depth"], 1e-4,
           1e-3 if bg_inf else 1e-4)
    if blend:
        _check(tag + " mpi_blend", got["blend"], ref["blend"], 1e-4, 1e-5)
    _check(tag + " grad_rgb", got["grad_rgb"], ref["grad_rgb"], 1e-3, 1e-3)
    _check(tag + " grad_sigma", got["grad_sigma"], ref["grad_sigma"],
           1e-3, 1e-3)


def _check_tgt(name, bg_inf, alpha, mode, monkeypatch):
    from mine_amd.ops import renderer
    monkeypatch.setattr(renderer, "_TGT_BWD_MODE", mode)
    got = _run_tgt(name, DEV, torch.float32, bg_inf, alpha)
    ref = _oracle_tgt(name, bg_inf, alpha)
    keep = _keep(name).unsqueeze(1)
    r = _bg_inf_ratio(name, alpha) if (bg_inf and not alpha) else 1.0
    tag = (f"tgt[{name} bg_inf={int(bg_inf)} alpha={int(alpha)} "
           f"mode={mode}]")
    print(f"{tag}: r = {r:.4g}, excluded = "
          f"{1.0 - keep.double().mean().item():.4f}")
    _check(tag + " rgb", got["rgb"], ref["rgb"], 1e-3, 1e-4, keep)
    if alpha:   # plain weighted z sum; atol of the suite's alpha test
        d_atol = 1e-2
    else:
        d_atol = 1e-2 if bg_inf else 1e-3
    _check(tag + " depth", got["depth"], ref["depth"], 1e-3, d_atol, keep)
    _check(tag + " mask", got["mask"], ref["mask"], 0.0, 0.5, keep)
    assert torch.equal(got["mask"][keep], ref["mask"][keep])
    _check(tag + " grad_rgb", got["grad_rgb"], ref["grad_rgb"], 1e-3, 1e-3)
    _check(tag + " grad_sigma", got["grad_sigma"], ref["grad_sigma"],
           1e-3, 1e-3 * r)


# ---------------------------------------------------------------------------
# CPU tests: the scenes have the properties the GPU tests rely on
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(_CASES))
def test_excluded_share_is_under_one_percent(name):
    keep = _keep(name)
    share = 1.0 - keep.double().mean(dim=(1, 2))
    print(f"{name}: excluded share per batch element = {share.tolist()}")
    assert float(share.max()) <= 0.01


def test_odd_scene_shape_properties():
    sc = _scene("odd")
    HW = sc["H"] * sc["W"]
    assert HW == 1665 and HW % 256 != 0
    assert (sc["W"] + GT - 1) // GT == 2 and (sc["H"] + GT - 1) // GT == 2
    assert sc["W"] % GT != 0 and sc["H"] % GT != 0
    assert sc["W"] // GT != (sc["W"] + GT - 1) // GT
    assert not torch.equal(sc["K"][0], sc["K"][1])
    assert not torch.equal(sc["disparity"][0], sc["disparity"][1])
    # strictly descending disparities, as the renderer expects
    for name in _CASES:
        d = _scene(name)["disparity"]
        assert bool((d[:, 1:] < d[:, :-1]).all()) and bool((d > 0).all())


def _src_acc(name):
    """Shifted transmittance product A_s of the source view, fp64."""
    sc = _scene(name)
    d64 = lambda t: t.double()
    grid = tr.make_meshgrid(sc["H"], sc["W"])
    xyz = tr.src_plane_xyz(grid, d64(sc["disparity"]), d64(sc["K_inv"]))
    _, _, acc, _ = tr.volume_composite(d64(sc["rgb"]), d64(sc["sigma"]),
                                       xyz, False)
    return acc[:, :, 0]  # (B,S,H,W)


def _tgt_acc(name):
    """The same for the target view: warp as render_tgt_reference does."""
    sc = _scene(name)
    B, S, H, W = sc["B"], sc["S"], sc["H"], sc["W"]
    d64 = lambda t: t.double()
    disp, G, Ki, K = (d64(sc[k]) for k in ("disparity", "G", "K_inv", "K"))
    grid = tr.make_meshgrid(H, W)
    xyz_tgt = tr.tgt_plane_xyz(tr.src_plane_xyz(grid, disp, Ki), G)
    planes = torch.cat((d64(sc["rgb"]), d64(sc["sigma"]), xyz_tgt), dim=2)
    hinv = tr.homography_tgt_to_src(G, torch.reciprocal(disp), Ki, K)
    warped, _ = tr.homography_grid_sample(planes.reshape(B * S, 7, H, W),
                                          hinv.reshape(B * S, 3, 3), H, W)
    warped = warped.reshape(B, S, 7, H, W)
    w_sigma = torch.where(warped[:, :, 6:7] >= 0, warped[:, :, 3:4],
                          torch.zeros_like(warped[:, :, 3:4]))
    _, _, acc, _ = tr.volume_composite(warped[:, :, 0:3], w_sigma,
                                       warped[:, :, 4:7], False)
    return acc[:, :, 0]


@pytest.mark.parametrize("view", ["src", "tgt"])
def test_exit_scene_dies_early_on_one_half_only(view):
    acc = _src_acc("exit") if view == "src" else _tgt_acc("exit")
    S = acc.shape[1]
    dead_early = (acc[:, 4] < DEAD).double().mean().item()
    never_dead = (acc[:, S - 1] >= DEAD).double().mean().item()
    # the exit happens right after plane 3, not before
    alive_at_3 = (acc[:, 3] >= DEAD).double().mean().item()
    print(f"exit[{view}]: dead before plane 4 = {dead_early:.3f}, never dead "
          f"= {never_dead:.3f}, alive entering plane 3 = {alive_at_3:.3f}")
    assert dead_early >= 0.40
    assert never_dead >= 0.40
    assert alive_at_3 >= 0.99
    assert S - 4 == 6  # six tail planes


def test_cull_scene_reaches_both_signs_of_z():
    sc = _scene("cull")
    u, v, z, hz = _geometry("cull")
    neg = (z < 0).double()
    share = neg.mean().item()
    per_plane = neg.mean(dim=(0, 2, 3))
    mixed = [(0.0 < p < 1.0) for p in per_plane.tolist()]
    print(f"cull: z<0 share = {share:.3f}, per plane = "
          f"{[round(p, 3) for p in per_plane.tolist()]}, "
          f"min|hz| = {hz.abs().min().item():.3f}")
    assert 0.10 <= share <= 0.60
    assert any(mixed)
    assert mixed[_CULL_DISP.index(0.5)]      # the plane at depth 2
    assert per_plane[:3].min().item() == 1.0  # nearest three: behind
    assert hz.abs().min().item() > 0.05
    assert sc["B"] == 1


@pytest.mark.parametrize("name", ["odd", "cull"])
def test_gather_bbox_fallback_is_taken_and_not_taken(name):
    fb = _fallback_tiles(name)
    print(f"{name}: fallback (b,s,tile) = {int(fb.sum())} of {fb.numel()}; "
          f"per (b,s) = {fb.sum(dim=2).tolist()}")
    assert bool(fb.any()) and bool((~fb).any())
    if name == "cull":  # the planes behind the camera supply it
        assert bool(fb[0, :3].all())
    # all geometry stays finite
    u, v, z, hz = _geometry(name)
    assert bool(torch.isfinite(u).all() and torch.isfinite(v).all())
    assert hz.abs().min().item() > 0.05


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("bg_inf", [False, True])
@pytest.mark.parametrize("blend", [False, True])
def test_src_odd_shape_matches_fp64_oracle(blend, bg_inf):
    _check_src("odd", blend, bg_inf)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("alpha", [False, True])
@pytest.mark.parametrize("bg_inf", [False, True])
def test_tgt_odd_shape_matches_fp64_oracle(bg_inf, alpha, mode, monkeypatch):
    _check_tgt("odd", bg_inf, alpha, mode, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bg_inf", [False, True])
@pytest.mark.parametrize("blend", [False, True])
@pytest.mark.parametrize("name", ["few1", "few2"])
def test_src_few_planes_matches_fp64_oracle(name, blend, bg_inf):
    _check_src(name, blend, bg_inf)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("bg_inf", [False, True])
@pytest.mark.parametrize("name", ["few1", "few2"])
def test_tgt_few_planes_matches_fp64_oracle(name, bg_inf, mode, monkeypatch):
    _check_tgt(name, bg_inf, False, mode, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("bg_inf", [False, True])
@pytest.mark.parametrize("blend", [False, True])
def test_src_deep_early_exit_matches_fp64_oracle(blend, bg_inf):
    """Six tail planes behind the exit: mpi_blend copy-through (forward)
    and the g_blend pass-through (backward) are compared plane by plane;
    additionally the tail must not be all zeros under blend."""
    _check_src("exit", blend, bg_inf)
    if blend:
        ref = _oracle_src("exit", blend, bg_inf)
        W = _scene("exit")["W"]
        tail = ref["grad_sigma"][:, 5:, :, :, :W // 2 - 1]
        assert tail.abs().median().item() > 0.1  # g_blend passes through


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("bg_inf", [False, True])
def test_tgt_deep_early_exit_matches_fp64_oracle(bg_inf, mode, monkeypatch):
    """The mask must count all 10 planes where the composite loop left at
    plane 3 (projection-only tail)."""
    _check_tgt("exit", bg_inf, False, mode, monkeypatch)
    ref = _oracle_tgt("exit", bg_inf, False)
    assert ref["mask"].max().item() == 10.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("bg_inf", [False, True])
def test_tgt_z_cull_matches_fp64_oracle(bg_inf, mode, monkeypatch):
    _check_tgt("cull", bg_inf, False, mode, monkeypatch)
    # culled planes get no sigma gradient at all in the oracle
    ref = _oracle_tgt("cull", bg_inf, False)
    assert ref["grad_sigma"][:, :3].abs().max().item() == 0.0
    assert ref["grad_sigma"][:, 3:].abs().max().item() > 0.0
