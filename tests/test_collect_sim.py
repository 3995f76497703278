"""CPU model of the collect pass of the order-fixed warp backward
(`tgt_collect_kernel`, render_kernels.hip): its search window and its
membership rule, replayed in fp32 with numpy.

For one plane the kernel gives every source texel an owner that visits a
window of target pixels and adds the taps that hit the texel. Membership
is `make_tap(project_uv(...))`, exactly what the scatter form uses; the
window is only a bound. The model below repeats both, operation by
operation, and the tests assert for every texel of every plane that

  * the window contains every target pixel that contributes (the exact
    set, from a brute-force pass over all pixels), and
  * the pull sum over the window, in raster order, equals the bilinear
    scatter in fp64 (both add the same fp64 products in the same order
    per texel, so equality is exact, dyadic data or not).

Planes: seeded random homographies plus one behind the camera (hz < 0
everywhere), one whose horizon crosses the image, one that minifies
below half a source pixel per target pixel, one that magnifies, one that
pushes more than a quarter of the target pixels over a border, and the
dyadic planes u = x/4 + c, v = y/2 + c' of the GPU tests. fp64 geometry
asserts each of these properties.

The second half asserts the properties of the scenes that
tests/test_deterministic_step_gpu.py relies on: a plane with a border-
clamped share above 25 %, a corner texel that receives more than one
clamped pixel, sparse-point sets with duplicates.
"""
import functools

import numpy as np
import pytest
import torch

from mine_amd.utils.geometry import inverse_3x3

F = np.float32


# ---------------------------------------------------------------------------
# fp32 replay of the device functions
# ---------------------------------------------------------------------------

def _fma(a, b, c):
    # one rounding: the fp32 product is exact in fp64
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(F)


def project_uv(Hm, xs, ys):
    """project_uv of render_kernels.hip; Hm (9,) fp32, xs/ys int arrays."""
    fx, fy = xs.astype(F), ys.astype(F)
    hx = _fma(Hm[0], fx, _fma(Hm[1], fy, Hm[2]))
    hy = _fma(Hm[3], fx, _fma(Hm[4], fy, Hm[5]))
    hz = _fma(Hm[6], fx, _fma(Hm[7], fy, Hm[8]))
    iz = F(1.0) / hz
    return hx * iz, hy * iz


def make_tap(u, v, W, H):
    """make_tap: clamp (fminf(fmaxf())), floor, +1 clamped, weights."""
    uc = np.fmin(np.fmax(u, F(0)), F(W - 1))
    vc = np.fmin(np.fmax(v, F(0)), F(H - 1))
    fx, fy = np.floor(uc), np.floor(vc)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    return x0, x1, y0, y1, (uc - fx).astype(F), (vc - fy).astype(F)


def contributions(Hm, H, W):
    """All (target pixel, texel, weight) triples of one plane in the
    scatter's order: pixels in raster order, tap kinds in scatter4's
    order, zero weights left out."""
    ys, xs = np.divmod(np.arange(H * W), W)
    u, v = project_uv(Hm, xs, ys)
    x0, x1, y0, y1, wx, wy = make_tap(u, v, W, H)
    one = F(1)
    w = np.stack(((one - wx) * (one - wy), wx * (one - wy),
                  (one - wx) * wy, wx * wy), axis=1)          # (HW,4) fp32
    q = np.stack((y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1), axis=1)
    pix = np.repeat(np.arange(H * W), 4).reshape(H * W, 4)
    keep = w != 0
    return pix[keep], q[keep], w[keep]


def _clip_row(a, c, m, W, lo, hi):
    """clip_row: returns (any, lo, hi)."""
    tiny = m / F(W)
    if a > tiny:
        xb = (-m - c) / a
        lo = max(lo, int(min(max(np.floor(xb), F(-1)), F(W))))
    elif a < -tiny:
        xb = (-m - c) / a
        hi = min(hi, int(min(max(np.ceil(xb), F(-1)), F(W))))
    elif c <= F(-2) * m:
        return False, lo, hi
    return lo <= hi, lo, hi


def window(Hi, Hf, H, W):
    """(HW texels, HW pixels) bool: the pixels each texel's owner visits.
    Mirrors tgt_collect_kernel line by line, in np.float32 scalars."""
    Hi = [F(x) for x in Hi]
    Hf = [F(x) for x in Hf]
    fW1, fH1 = F(W - 1), F(H - 1)
    Tx = abs(Hi[0]) * fW1 + abs(Hi[1]) * fH1 + abs(Hi[2])
    Ty = abs(Hi[3]) * fW1 + abs(Hi[4]) * fH1 + abs(Hi[5])
    Tz = abs(Hi[6]) * fW1 + abs(Hi[7]) * fH1 + abs(Hi[8])
    finite = bool(np.isfinite(Tx + Ty + Tz))
    mz = F(1e-5) * Tz
    out = np.zeros((H * W, H, W), dtype=bool)
    for q in range(H * W):
        qy, qx = divmod(q, W)
        c_ul, c_uh, c_vl, c_vh = qx > 0, qx < W - 1, qy > 0, qy < H - 1
        ylo, yhi = 0, H - 1
        if finite and c_ul and c_uh and c_vl and c_vh:
            pos = neg = fin = True
            mny, mxy = F(1e30), F(-1e30)
            for cy in (F(qy) - F(1.25), F(qy) + F(1.25)):
                for cx in (F(qx) - F(1.25), F(qx) + F(1.25)):
                    pz = Hf[6] * cx + Hf[7] * cy + Hf[8]
                    py = (Hf[3] * cx + Hf[4] * cy + Hf[5]) / pz
                    pos = pos and pz > F(1e-8)
                    neg = neg and pz < F(-1e-8)
                    fin = fin and bool(np.isfinite(py))
                    mny, mxy = np.fmin(mny, py), np.fmax(mxy, py)
            if (pos or neg) and fin:
                ylo = int(min(max(np.floor(mny - F(1)), F(0)), fH1))
                yhi = int(min(max(np.ceil(mxy + F(1)), F(0)), fH1))
        for y in range(ylo, yhi + 1):
            lo, hi = 0, W - 1
            fy = F(y)
            hz0 = Hi[7] * fy + Hi[8]
            hz1 = Hi[6] * fW1 + hz0
            sg = F(0)
            if finite:
                if hz0 > mz and hz1 > mz:
                    sg = F(1)
                elif hz0 < -mz and hz1 < -mz:
                    sg = F(-1)
            if sg != 0:
                ok = True
                for cond, k, sgn, r, T in (
                        (c_ul, F(qx - 1), F(1), 0, Tx),
                        (c_uh, F(qx + 1), F(-1), 0, Tx),
                        (c_vl, F(qy - 1), F(1), 3, Ty),
                        (c_vh, F(qy + 1), F(-1), 3, Ty)):
                    if ok and cond:
                        a = sgn * sg * (Hi[r] - k * Hi[6])
                        c = sgn * sg * ((Hi[r + 1] - k * Hi[7]) * fy +
                                        (Hi[r + 2] - k * Hi[8]))
                        m = F(1e-5) * (T + (abs(k) + F(1)) * Tz)
                        ok, lo, hi = _clip_row(a, c, m, W, lo, hi)
                if not ok:
                    continue
                lo, hi = max(lo, 0), min(hi, W - 1)
            out[q, y, lo:hi + 1] = True
    return out.reshape(H * W, H * W)


# ---------------------------------------------------------------------------
# planes
# ---------------------------------------------------------------------------

SIM_H, SIM_W = 11, 14


def _mat(a, b, c, d, e, f, g, h, i=1.0):
    return np.array([a, b, c, d, e, f, g, h, i], dtype=F)


def dyadic_hinv(offsets):
    """(len(offsets), 3, 3) fp32 tensors of u = x/4 + c, v = y/2 + c'."""
    out = torch.zeros(len(offsets), 3, 3)
    for i, (c, cp) in enumerate(offsets):
        out[i] = torch.tensor([[0.25, 0.0, c], [0.0, 0.5, cp],
                               [0.0, 0.0, 1.0]])
    return out


# offsets of the GPU tests' dyadic planes; between them they clamp on all
# four sides (asserted below)
DYADIC_37x45 = [(-2.25, -1.5), (40.5, 30.25), (-1.75, 25.5),
                (38.25, -3.5), (3.5, 5.25), (-0.5, 33.75)]
DYADIC_9x11 = [(-1.25, -1.5), (8.75, 5.5)]


def _sim_planes():
    H, W = SIM_H, SIM_W
    rng = np.random.RandomState(11)
    planes = {}
    for i in range(3):
        r = rng.uniform(-1, 1, 8)
        planes[f"random{i}"] = _mat(1 + 0.2 * r[0], 0.1 * r[1], 3 * r[2],
                                    0.1 * r[3], 1 + 0.2 * r[4], 3 * r[5],
                                    0.005 * r[6], 0.005 * r[7])
    planes["behind"] = -planes["random0"]
    planes["horizon"] = _mat(1.0, 0.05, 0.5, -0.03, 1.0, 0.25,
                             -1.0 / 7.5, 0.01)
    planes["minify"] = _mat(0.3, 0.02, 4.0, -0.01, 0.35, 3.0, 0.001, -0.002)
    planes["magnify"] = _mat(2.6, 0.1, -9.0, 0.2, 3.1, -8.0, 0.002, 0.001)
    planes["border"] = _mat(1.0, 0.03, -0.45 * W, 0.02, 1.0, 1.5,
                            0.001, 0.0)
    planes["dyadic0"] = dyadic_hinv([(-1.25, -1.5)])[0].numpy().reshape(9)
    planes["dyadic1"] = dyadic_hinv([(11.75, 7.5)])[0].numpy().reshape(9)
    return planes


PLANES = _sim_planes()


def _fwd(Hm):
    return inverse_3x3(torch.from_numpy(Hm.reshape(1, 3, 3))) \
        .reshape(9).numpy().astype(F)


def _geometry64(Hm, H, W):
    ys, xs = np.divmod(np.arange(H * W), W)
    h = Hm.astype(np.float64)
    hz = h[6] * xs + h[7] * ys + h[8]
    with np.errstate(all="ignore"):
        u = (h[0] * xs + h[1] * ys + h[2]) / hz
        v = (h[3] * xs + h[4] * ys + h[5]) / hz
    return u, v, hz


def _clamped(u, v, H, W):
    return (u < 0) | (u > W - 1) | (v < 0) | (v > H - 1)


def test_planes_have_the_advertised_properties():
    H, W = SIM_H, SIM_W
    _, _, hz = _geometry64(PLANES["behind"], H, W)
    assert (hz < 0).all()
    _, _, hz = _geometry64(PLANES["horizon"], H, W)
    assert (hz > 0).any() and (hz < 0).any()
    m = PLANES["minify"].astype(np.float64)
    u, v, _ = _geometry64(PLANES["minify"], H, W)
    du = np.abs(np.diff(u.reshape(H, W), axis=1))
    dv = np.abs(np.diff(v.reshape(H, W), axis=0))
    assert du.max() < 0.5 and dv.max() < 0.5, (du.max(), dv.max(), m)
    u, v, _ = _geometry64(PLANES["magnify"], H, W)
    assert np.abs(np.diff(u.reshape(H, W), axis=1)).min() > 2.0
    u, v, _ = _geometry64(PLANES["border"], H, W)
    share = _clamped(u, v, H, W).mean()
    print(f"border plane: clamped share = {share:.3f}")
    assert share > 0.25


@pytest.mark.parametrize("name", sorted(PLANES))
def test_window_contains_the_contributing_set_and_pull_equals_scatter(name):
    H, W = SIM_H, SIM_W
    Hi = PLANES[name]
    with np.errstate(all="ignore"):
        pix, tex, w = contributions(Hi, H, W)
        win = window(Hi, _fwd(Hi), H, W)
    inside = win[tex, pix]
    missed = int((~inside).sum())
    sizes = win.sum(axis=1).reshape(H, W)
    print(f"{name}: {len(pix)} contributions, {missed} outside their "
          f"window; window size interior median = "
          f"{np.median(sizes[1:-1, 1:-1]):.0f}, ring max = "
          f"{max(sizes[0].max(), sizes[-1].max(), sizes[:, 0].max(), sizes[:, -1].max())}"
          f" of {H * W}")
    assert missed == 0

    g = np.random.RandomState(5).randint(-8, 9, size=H * W).astype(np.float64)
    val = w.astype(np.float64) * g[pix]
    scatter = np.zeros(H * W)
    np.add.at(scatter, tex, val)       # unbuffered: in the order given
    pull = np.zeros(H * W)
    np.add.at(pull, tex[inside], val[inside])
    assert np.array_equal(pull, scatter)
    if name.startswith("dyadic"):
        # every weight a multiple of 1/8: any order is exact, also in fp32
        assert np.array_equal(val, np.round(val * 8) / 8)
        assert torch.equal(torch.from_numpy(pull).float().double(),
                           torch.from_numpy(scatter))
    if name in ("random0", "random1", "random2", "dyadic0", "magnify"):
        # the window is a bound, but not a useless one
        assert np.median(sizes[1:-1, 1:-1]) <= H * W / 4


def test_non_finite_plane_scans_everything():
    H, W = 5, 6
    Hi = _mat(1.0, 0.0, np.nan, 0.0, 1.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        win = window(Hi, _fwd(Hi), H, W)
    assert win.all()


# ---------------------------------------------------------------------------
# scenes of tests/test_deterministic_step_gpu.py
# ---------------------------------------------------------------------------

def scatter_reference(payload, hinv):
    """fp64 bilinear scatter of `payload` (B,S,H,W,4) through hinv
    (B,S,3,3), the fp64 form of scatter4: border-clamped taps, zero
    weights left out. Returns (B,S,H,W,4) fp64."""
    B, S, H, W, _ = payload.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64),
                            torch.arange(W, dtype=torch.float64),
                            indexing="ij")
    p = torch.stack((xs, ys, torch.ones_like(xs))).reshape(3, -1)
    m = torch.matmul(hinv.double(), p)                       # (B,S,3,HW)
    u = (m[:, :, 0] / m[:, :, 2]).clamp(0, W - 1)
    v = (m[:, :, 1] / m[:, :, 2]).clamp(0, H - 1)
    x0, y0 = u.floor(), v.floor()
    wx, wy = u - x0, v - y0
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    out = torch.zeros(B, S, H * W, 4, dtype=torch.float64)
    pay = payload.double().reshape(B, S, H * W, 4)
    for qx, qy, wgt in ((x0, y0, (1 - wx) * (1 - wy)), (x1, y0, wx * (1 - wy)),
                        (x0, y1, (1 - wx) * wy), (x1, y1, wx * wy)):
        idx = (qy * W + qx).unsqueeze(-1).expand(B, S, H * W, 4)
        out.scatter_add_(2, idx, wgt.unsqueeze(-1) * pay)
    return out.reshape(B, S, H, W, 4)


@pytest.mark.parametrize("shape,offsets", [((37, 45), DYADIC_37x45),
                                           ((9, 11), DYADIC_9x11)])
def test_dyadic_planes_clamp_on_all_four_sides(shape, offsets):
    H, W = shape
    sides = dict(left=False, right=False, top=False, bottom=False)
    best, corner = 0.0, 0
    for hm in dyadic_hinv(offsets):
        u, v, _ = _geometry64(hm.numpy().reshape(9), H, W)
        sides["left"] |= bool((u < 0).any())
        sides["right"] |= bool((u > W - 1).any())
        sides["top"] |= bool((v < 0).any())
        sides["bottom"] |= bool((v > H - 1).any())
        best = max(best, _clamped(u, v, H, W).mean())
        corner = max(corner, int(((u <= 0) & (v <= 0)).sum()),
                     int(((u >= W - 1) & (v >= H - 1)).sum()))
        # exact in fp32: quarter-pixel coordinates
        assert np.array_equal(u * 4, np.round(u * 4))
        assert np.array_equal(v * 4, np.round(v * 4))
    print(f"{H}x{W}: sides {sides}, largest clamped share {best:.3f}, "
          f"most pixels on one corner texel {corner}")
    assert all(sides.values())
    assert best > 0.25
    assert corner > 1


def sparse_points(seed=3, B=2, H=8, W=12, N=128):
    """Bx2xN pixel coordinates, some outside the image."""
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(B, N, generator=g) * (W + 3) - 2.0
    py = torch.rand(B, N, generator=g) * (H + 3) - 2.0
    return torch.stack((px, py), dim=1)


def flat_index(pxpy, H, W):
    pp = torch.round(pxpy).to(torch.int64)
    return pp[:, 0].clamp(0, W - 1) + W * pp[:, 1].clamp(0, H - 1)


def test_sparse_points_contain_duplicates_and_outsiders():
    H, W = 8, 12
    pxpy = sparse_points()
    idx = flat_index(pxpy, H, W)
    for b in range(idx.shape[0]):
        assert idx[b].unique().numel() < idx.shape[1]
    counts = torch.bincount(idx[0], minlength=H * W)
    print(f"sparse points: most points on one pixel = {int(counts.max())}")
    assert int(counts.max()) >= 3  # more than two addends: order matters
    outside = (pxpy[:, 0] < -0.5) | (pxpy[:, 0] > W - 0.5) | \
        (pxpy[:, 1] < -0.5) | (pxpy[:, 1] > H - 0.5)
    assert bool(outside.any())


def test_sparse_module_matches_reference_on_cpu():
    from mine_amd.ops import gather_pixel_by_pxpy, torch_ref
    from mine_amd.ops.sparse import _flat_index
    img = torch.arange(2 * 3 * 8 * 12, dtype=torch.float32).reshape(2, 3, 8, 12)
    pxpy = sparse_points()
    assert torch.equal(gather_pixel_by_pxpy(img, pxpy),
                       torch_ref.gather_pixel_by_pxpy(img, pxpy))
    assert torch.equal(_flat_index(pxpy, 8, 12), flat_index(pxpy, 8, 12))


def test_sobel_from_slices_matches_conv_form():
    from mine_amd.ops.losses import _spatial_gradient_slices, spatial_gradient
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 7, 9, generator=g, dtype=torch.float64,
                    ).requires_grad_(True)
    up = torch.randn(2, 3, 2, 7, 9, generator=g, dtype=torch.float64)
    for normalized in (True, False):
        a = spatial_gradient(x, normalized)
        b = _spatial_gradient_slices(x, normalized)
        torch.testing.assert_close(b, a, rtol=1e-13, atol=1e-13)
        ga, = torch.autograd.grad((a * up).sum(), x)
        gb, = torch.autograd.grad((b * up).sum(), x)
        torch.testing.assert_close(gb, ga, rtol=1e-13, atol=1e-13)


# the whole-step scene: synthetic 128x192 batch with the target camera
# yawed, so that a quarter of the image is border-clamped on every plane
# whatever scale factor the step derives for the translation
STEP_H, STEP_W, STEP_B, STEP_S, STEP_NPT = 128, 192, 2, 8, 128
STEP_POSE = ((0.05, 0.32, 0.04), (0.12, -0.05, 0.03))  # axis-angle, t


def step_config(**extra):
    from mine_amd.config import default_config
    over = {
        "data.name": "synthetic", "data.img_h": STEP_H, "data.img_w": STEP_W,
        "mpi.num_bins_coarse": STEP_S, "data.per_gpu_batch_size": STEP_B,
        "data.visible_point_count": STEP_NPT, "data.num_workers": 0,
        "loss.smoothness_lambda_v1": 0.5,
        "training.deterministic": True,
    }
    over.update(extra)
    return default_config(**over)


@functools.lru_cache(maxsize=None)
def step_items():
    from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
    from test_render_paths_gpu import _rodrigues
    cfg = step_config()
    ds = SyntheticMPIDataset(cfg, length=STEP_B)
    src, tgt = collate_src_tgt([ds[i] for i in range(STEP_B)])
    G = torch.eye(4)
    G[:3, :3] = _rodrigues(torch.tensor(STEP_POSE[0]))
    G[:3, 3] = torch.tensor(STEP_POSE[1])
    tgt["G_src_tgt"] = G.view(1, 1, 4, 4).repeat(STEP_B, 1, 1, 1)
    return src, tgt


def test_step_scene_clamps_and_has_duplicate_points():
    from mine_amd.ops import torch_ref as tr
    from mine_amd.utils.geometry import inverse_rigid_4x4
    cfg = step_config()
    src, tgt = step_items()
    assert cfg["loss.smoothness_lambda_v1"] != 0.0
    K = src["K"].double()
    G_tgt_src = inverse_rigid_4x4(tgt["G_src_tgt"][:, 0]).double()
    H, W = STEP_H, STEP_W
    disp = torch.linspace(float(cfg["mpi.disparity_start"]),
                          float(cfg["mpi.disparity_end"]), STEP_S,
                          dtype=torch.float64).repeat(STEP_B, 1)
    # the step divides t by a scale factor it derives from the network
    # output; the yaw keeps the share at every factor
    for sf in (0.25, 1.0, 4.0):
        G = G_tgt_src.clone()
        G[:, :3, 3] /= sf
        hinv = tr.homography_tgt_to_src(G, torch.reciprocal(disp),
                                        torch.inverse(K), K)
        shares, corner = [], 0
        for s in range(STEP_S):
            u, v, _ = _geometry64(hinv[0, s].numpy().reshape(9), H, W)
            shares.append(_clamped(u, v, H, W).mean())
            for cu in (u <= 0, u >= W - 1):
                for cv in (v <= 0, v >= H - 1):
                    corner = max(corner, int((cu & cv).sum()))
        print(f"sf={sf}: clamped share per plane = "
              f"{[round(float(x), 3) for x in shares]}, most pixels on one "
              f"corner texel = {corner}")
        assert min(shares) > 0.25
        assert corner > 1
    # sparse points: duplicates at the coarse scales
    for key, pts in (("src", src["xyzs"]), ("tgt", tgt["xyzs"][:, 0])):
        for scale in (2, 3):
            Hs, Ws = H >> scale, W >> scale
            Ks = src["K"].clone()
            Ks[:, 0] *= Ws / W
            Ks[:, 1] *= Hs / H
            p = torch.matmul(Ks, pts)
            idx = flat_index(p[:, 0:2] / p[:, 2:], Hs, Ws)
            for b in range(STEP_B):
                dup = idx.shape[1] - idx[b].unique().numel()
                assert dup > 0, (key, scale, b)
