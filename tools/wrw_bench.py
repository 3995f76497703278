"""Per-shape timing of the conv3x3 weight gradient (ext.conv3x3_wrw) at
the flagship decoder's eight layers, as effective bandwidth.

    python tools/wrw_bench.py [--root OTHER_CHECKOUT] [--miopen] [--bias]
                              [--dtype {bf16,fp16}]

Times are device-event medians of the whole binding call (workspace or
zero fill, the kernel, the finishing kernel). Effective TB/s = compulsory
bytes / time, the bytes computed here from the shapes: x and gy read once
(the output is at most 64x64x9 floats). The ceiling printed next to each
is what the fused BN+activation forward kernel (one read + one write of
the larger tensor) reaches in the same session.

--root imports mine_amd from another built checkout, so two builds can be
timed with the same shape list. --bias times the (dw, db) binding where
the build has it. --miopen also times the library weight gradient on a
padded copy.
"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--miopen", action="store_true")
ap.add_argument("--bias", action="store_true")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
import torch.nn.functional as F
from mine_amd.ops.backend import get_extension

DTYPE = torch.float16 if args.dtype == "fp16" else torch.bfloat16

N = 256  # B*S of the flagship config
SHAPES = [  # (name, C, H, W, K)
    ("upconv(2,1) dec", 64, 64, 96, 64),
    ("dispconv 2", 64, 64, 96, 4),
    ("upconv(1,0)", 64, 64, 96, 32),
    ("upconv(1,1) dec", 32, 128, 192, 32),
    ("dispconv 1", 32, 128, 192, 4),
    ("upconv(0,0)", 32, 128, 192, 16),
    ("upconv(0,1)", 16, 256, 384, 16),
    ("dispconv 0", 16, 256, 384, 4),
]


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


_BN_RATE = {}


def bn_rate(nbytes):
    """TB/s of bn_act_fwd (1 read + 1 write) on a DTYPE tensor of nbytes."""
    if nbytes not in _BN_RATE:
        C = 16
        M = nbytes // (2 * C)
        x = torch.randn(M * C, device="cuda:0", dtype=DTYPE)
        z = torch.zeros(C, device="cuda:0")
        o = torch.ones(C, device="cuda:0")
        res = torch.empty(0, device="cuda:0", dtype=DTYPE)
        t = tm(lambda: ext.bn_act_fwd(x, res, z, o, o, z, M, C, 3), args.reps)
        _BN_RATE[nbytes] = 2 * nbytes / t / 1e9
    return _BN_RATE[nbytes]


ext = get_extension(required=True)
call = ext.conv3x3_wrw
if args.bias:
    call = ext.conv3x3_wrw_bias   # an error on builds without it
reps = max(args.reps, 8)
total = total_mi = 0.0
print(f"root {args.root}  binding {call.__name__}  dtype {args.dtype}")
print(f"{'layer':<16} {'C->K':>7} {'HxW':>9} | {'wrw ms':>7} {'GB':>5} "
      f"{'TB/s':>5} {'ceil':>5} {'%':>4}")
for (name, C, H, W, K) in SHAPES:
    x = torch.randn(N, C, H, W, device="cuda:0", dtype=DTYPE
                    ).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(N, K, H, W, device="cuda:0", dtype=DTYPE
                     ).contiguous(memory_format=torch.channels_last)
    xf = x.permute(0, 2, 3, 1).reshape(-1)
    gf = gy.permute(0, 2, 3, 1).reshape(-1)
    t = tm(lambda: call(xf, gf, N, H, W, C, K), reps)
    by_x, by_gy = x.numel() * 2, gy.numel() * 2
    rate = (by_x + by_gy) / t / 1e9
    ceil = bn_rate(max(by_x, by_gy))
    extra = ""
    if args.miopen:
        xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
        w = torch.randn(K, C, 3, 3, device="cuda:0", dtype=DTYPE)
        t_mi = tm(lambda: torch.ops.aten.convolution_backward(
            gy, xp, w, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
            [False, True, False]), reps)
        total_mi += t_mi
        extra = f" | miopen {t_mi:7.3f}"
        del xp
    print(f"{name:<16} {C:>3}->{K:<3} {H:>4}x{W:<4} | {t:7.3f} "
          f"{(by_x + by_gy) / 1e9:5.2f} {rate:5.2f} {ceil:5.2f} "
          f"{100 * rate / ceil:4.0f}{extra}")
    total += t
    del x, gy, xf, gf
print(f"TOTAL wrw {total:.2f} ms" +
      (f"  miopen {total_mi:.2f} ms" if args.miopen else ""))
