"""Per-scale timing of the novel-view renderer (forward, and the gather-mode
backward: backward kernel + gather kernel + zero fills) at the flagship's
four scales, as effective bandwidth.

    python tools/render_bench.py [--root OTHER_CHECKOUT] [--reps 9]
                                 [--scales 0,1,2,3] [--only {all,fwd,bwd}]
                                 [--no-split] [--mode {1,2}] [--views V]

B = 4, S = 64, fp32 MPI (B,S,H,W,4) at 256x384, 128x192, 64x96, 32x48.
Seeded inputs: small camera motion, and sigma small enough that the
transmittance stays alive down to the far plane, as in a step from random
initialisation (no early exit shortens the per-pixel loops).

Call times are device-event medians. The split of the backward call into
its two kernels comes from the device durations torch.profiler records
over the same number of calls, taken after the event timing (medians per
kernel name). The fills are timed as one `zeros_like(mpi)`; a build whose
binding takes `workspace` fills once per call (grad_mpi), an older one
twice (grad_mpi and payload).

Effective TB/s = compulsory bytes / time, with N = bytes of the MPI:
forward N (one read), backward kernel 2N (read MPI, write payload), gather
kernel 2N (read payload, write grad_mpi), fill N. The ceiling printed next
to them is what the fused BN+activation forward kernel (one read + one
write) reaches on a tensor of N bytes in the same process.

--mode 2 times the order-fixed backward of deterministic mode instead:
the emit instance of the backward kernel, `tgt_collect_kernel` in the
gather kernel's place, and no fill at all.

--views V times the view-batched op instead (V cameras on a small circle
around the scene's pose, all reading the one MPI): `tgt_views_fwd` and
`tgt_views_bwd` in --mode, each against V calls of the single-view
binding on the same geometry, and the peak memory either backward
allocates on top of its inputs.

--root imports mine_amd from another built checkout, so two builds can be
timed with the same scenes. --only and --scales narrow the run to a few
dispatches for a counter collection.
"""
import argparse, inspect, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scales", default="0,1,2,3")
ap.add_argument("--only", choices=("all", "fwd", "bwd"), default="all")
ap.add_argument("--no-split", action="store_true")
ap.add_argument("--mode", type=int, choices=(1, 2), default=1)
ap.add_argument("--views", type=int, default=0)
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
from mine_amd.ops.backend import get_extension
from mine_amd.ops import torch_ref as tr
from mine_amd.utils.geometry import inverse_3x3

DEV = "cuda:0"
B, S = 4, 64
SCALES = [(256, 384), (128, 192), (64, 96), (32, 48)]
ext = get_extension(required=True)
HAS_WS = "workspace" in (ext.tgt_composite_bwd.__doc__ or "")
N_FILLS = 0 if args.mode == 2 else (1 if HAS_WS else 2)
PULL = "tgt_collect_kernel" if args.mode == 2 else "tgt_gather_kernel"


def tm(fn, reps):
    """Median device-event time in ms over `reps` calls after warm-up."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def bn_rate(nbytes):
    """TB/s of bn_act_fwd (1 read + 1 write) on a bf16 tensor of nbytes."""
    C = 16
    M = nbytes // (2 * C)
    x = torch.randn(M * C, device=DEV, dtype=torch.bfloat16)
    z = torch.zeros(C, device=DEV)
    o = torch.ones(C, device=DEV)
    res = torch.empty(0, device=DEV, dtype=torch.bfloat16)
    t = tm(lambda: ext.bn_act_fwd(x, res, z, o, o, z, M, C, 3), args.reps)
    return 2 * nbytes / t / 1e9


def scene(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.rand(B, S, H, W, 3, generator=g)
    sigma = torch.rand(B, S, H, W, 1, generator=g) * 0.05 + 1e-4
    mpi = torch.cat((rgb, sigma), dim=-1).to(DEV).contiguous()
    disp = torch.linspace(0.999, 0.05, S).unsqueeze(0).repeat(B, 1)
    depths = torch.reciprocal(disp).to(DEV).contiguous()
    f = 0.8 * W
    K = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])
    K = K.unsqueeze(0).repeat(B, 1, 1).to(DEV)
    K_inv = torch.inverse(K)
    G = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
    aa = 0.01 * torch.randn(B, 3, generator=g)
    for b in range(B):  # small rotation (first order) + small translation
        G[b, 0, 1], G[b, 1, 0] = -aa[b, 2], aa[b, 2]
        G[b, 0, 2], G[b, 2, 0] = aa[b, 1], -aa[b, 1]
        G[b, 1, 2], G[b, 2, 1] = -aa[b, 0], aa[b, 0]
        G[b, :3, 3] = 0.05 * torch.randn(3, generator=g)
    G = G.to(DEV)
    hinv = tr.homography_tgt_to_src(G, depths, K_inv, K).contiguous()
    m = torch.matmul(G[:, :3, :3], K_inv).contiguous()
    tvec = G[:, :3, 3].contiguous()
    hfwd = inverse_3x3(hinv.reshape(-1, 3, 3)).reshape(B, S, 3, 3).contiguous()
    g_rgb = torch.randn(B, 3, H, W, generator=g).to(DEV)
    g_depth = torch.randn(B, 1, H, W, generator=g).to(DEV)
    return mpi, depths, hinv, hfwd, m, tvec, g_rgb, g_depth


def views_scene(H, W, seed, V):
    """scene() plus V view-major poses: the scene's pose moved along a small
    circle (radius 0.03), as neighbouring frames of a video trajectory."""
    import math
    mpi, depths, hinv0, _, _, _, _, _ = scene(H, W, seed)
    g = torch.Generator().manual_seed(seed + 50)
    f = 0.8 * W
    K = torch.tensor([[f, 0.0, W / 2], [0.0, f, H / 2], [0.0, 0.0, 1.0]])
    K = K.unsqueeze(0).repeat(B, 1, 1).to(DEV)
    K_inv = torch.inverse(K)
    G = torch.eye(4).repeat(V, B, 1, 1)
    for v in range(V):
        a = 2.0 * math.pi * v / V
        G[v, :, 0, 3] = 0.03 * math.sin(a)
        G[v, :, 1, 3] = 0.03 * math.cos(a)
        G[v, :, 2, 3] = 0.02 * v / V
    G = G.to(DEV).reshape(V * B, 4, 4)
    K_si = K_inv.repeat(V, 1, 1)
    hinv = tr.homography_tgt_to_src(G, depths.repeat(V, 1), K_si,
                                    K.repeat(V, 1, 1))
    hfwd = inverse_3x3(hinv.reshape(-1, 3, 3))
    shape = lambda t, *tail: t.reshape(V, B, *tail).contiguous()
    g_rgb = torch.randn(V, B, 3, H, W, generator=g).to(DEV)
    g_depth = torch.randn(V, B, 1, H, W, generator=g).to(DEV)
    return (mpi, depths, shape(hinv, S, 3, 3), shape(hfwd, S, 3, 3),
            shape(torch.matmul(G[:, :3, :3], K_si), 3, 3),
            shape(G[:, :3, 3], 3), g_rgb, g_depth)


def peak_extra(fn):
    """Peak bytes `fn` allocates on top of what is live before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def run_views(V):
    print(f"root {args.root}")
    print(f"view-batched op against {V} single-view calls, backward mode "
          f"{args.mode}")
    print(f"{'HxW':>9} {'N MB':>6} | {'what':<10} {'views ms':>9} "
          f"{'single ms':>9} {'ratio':>6} | peak extra MB: views, single")
    for si in [int(v) for v in args.scales.split(",")]:
        H, W = SCALES[si]
        mpi, depths, hinv, hfwd, m, tvec, g_rgb, g_depth = \
            views_scene(H, W, 100 + si, V)
        N = mpi.numel() * 4
        vb = ext._views

        def fwd_v():
            return vb.tgt_views_fwd(mpi, hinv, m, tvec, depths, V, False,
                                    False)

        def fwd_1():
            return [ext.tgt_composite_fwd(mpi, hinv[v], m[v], tvec[v],
                                          depths, False, False)
                    for v in range(V)]

        def bwd_v():
            return vb.tgt_views_bwd(mpi, hinv, hfwd, m, tvec, depths, V,
                                    False, False, g_rgb, g_depth, args.mode)

        def bwd_1():
            # what autograd does with V single-view ops: V gradients of the
            # size of the MPI, summed
            total = None
            for v in range(V):
                g = ext.tgt_composite_bwd(mpi, hinv[v], hfwd[v], m[v],
                                          tvec[v], depths, False, False,
                                          g_rgb[v], g_depth[v], args.mode)
                total = g if total is None else total.add_(g)
            return total

        with torch.no_grad():
            for what, fv, f1 in (("fwd", fwd_v, fwd_1), ("bwd", bwd_v, bwd_1)):
                if args.only not in ("all", what):
                    continue
                tv, t1 = tm(fv, args.reps), tm(f1, args.reps)
                pv, p1 = peak_extra(fv), peak_extra(f1)
                print(f"{H:>4}x{W:<4} {N / 1e6:6.1f} | {what:<10} {tv:9.3f} "
                      f"{t1:9.3f} {tv / t1:6.2f} | {pv / 1e6:8.1f} "
                      f"{p1 / 1e6:8.1f}")
        del mpi


if args.views > 0:
    run_views(args.views)
    sys.exit(0)


def kernel_split(fn, reps):
    """Median device duration in ms per kernel name over `reps` calls."""
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    per = {}
    for ev in p.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            for key in ("tgt_composite_bwd_kernel", PULL):
                if key in ev.name:
                    per.setdefault(key, []).append(ev.device_time / 1e3)
    return {k: sorted(v)[len(v) // 2] for k, v in per.items()}


print(f"root {args.root}")
print(f"mode {args.mode}; binding takes workspace: {HAS_WS} -> {N_FILLS} "
      f"zero fill(s) per call")
print(f"{'HxW':>9} {'N MB':>6} {'ceil':>5} | {'what':<14} {'ms':>7} {'TB/s':>5} "
      f"{'%ceil':>5}")
tot = {}
for si in [int(v) for v in args.scales.split(",")]:
    H, W = SCALES[si]
    mpi, depths, hinv, hfwd, m, tvec, g_rgb, g_depth = scene(H, W, 100 + si)
    N = mpi.numel() * 4
    ceil = bn_rate(N)
    rows = []
    with torch.no_grad():
        if args.only in ("all", "fwd"):
            t = tm(lambda: ext.tgt_composite_fwd(mpi, hinv, m, tvec, depths,
                                                 False, False), args.reps)
            rows.append(("fwd", t, N))
        if args.only in ("all", "bwd"):
            bwd = lambda: ext.tgt_composite_bwd(mpi, hinv, hfwd, m, tvec,
                                                depths, False, False, g_rgb,
                                                g_depth, args.mode)
            t = tm(bwd, args.reps)
            rows.append(("bwd call", t, (4 + N_FILLS) * N))
            if N_FILLS:
                tf = tm(lambda: torch.zeros_like(mpi), args.reps)
                rows.append((f"fill x{N_FILLS}", N_FILLS * tf, N_FILLS * N))
            if not args.no_split:
                sp = kernel_split(bwd, args.reps)
                rows.append(("bwd kernel", sp["tgt_composite_bwd_kernel"],
                             2 * N))
                rows.append((PULL[4:].replace("_", " "), sp[PULL], 2 * N))
    for what, t, nbytes in rows:
        rate = nbytes / t / 1e9
        print(f"{H:>4}x{W:<4} {N / 1e6:6.1f} {ceil:5.2f} | {what:<14} {t:7.3f} "
              f"{rate:5.2f} {100 * rate / ceil:5.0f}")
        tot[what] = tot.get(what, 0.0) + t
    del mpi
print("TOTAL over the scales run: " +
      "  ".join(f"{k} {v:.3f} ms" for k, v in tot.items()))
