"""Per-shape timing of the MFMA conv3x3 forward and data gradient at the
flagship decoder's eight layers, as effective bandwidth.

    python tools/conv_bench.py [--root OTHER_CHECKOUT] [--miopen]
                               [--dtype {bf16,fp16}]

Times are device-event medians. Effective TB/s = compulsory bytes / time,
the bytes computed here from the shapes: the forward reads x and writes
y once; the data gradient (zero-embed conv + reflect fold, two kernels)
reads gy and writes gx once — its (H+2)x(W+2) intermediate is not
compulsory and is not counted. The ceiling printed next to each is what
the fused BN+activation forward kernel (one read + one write of the same
tensor size) reaches in the same session.

--root imports mine_amd from another built checkout, so two builds can be
timed with the same shape list. --miopen also times pad + library conv.
"""
import argparse, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--miopen", action="store_true")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
import torch.nn.functional as F
from mine_amd.ops.backend import get_extension
from mine_amd.ops.conv import conv3x3_reflect, conv3x3_bwd_data

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
        ext = get_extension(required=True)
        C = 16
        M = nbytes // (2 * C)
        x = torch.randn(M * C, device="cuda:0", dtype=DTYPE)
        z = torch.zeros(C, device="cuda:0")
        o = torch.ones(C, device="cuda:0")
        res = torch.empty(0, device="cuda:0", dtype=DTYPE)
        t = tm(lambda: ext.bn_act_fwd(x, res, z, o, o, z, M, C, 3), args.reps)
        _BN_RATE[nbytes] = 2 * nbytes / t / 1e9
    return _BN_RATE[nbytes]


reps = max(args.reps, 8)
print(f"dtype {args.dtype}")
tot = {"fwd": 0.0, "bwd": 0.0}
print(f"{'layer':<16} {'C->K':>7} {'HxW':>9} | {'fwd ms':>7} {'TB/s':>5} "
      f"{'ceil':>5} {'%':>4} | {'bwdD ms':>7} {'TB/s':>5} {'ceil':>5} {'%':>4}")
for (name, C, H, W, K) in SHAPES:
    x = torch.randn(N, C, H, W, device="cuda:0", dtype=DTYPE
                    ).contiguous(memory_format=torch.channels_last)
    w = torch.randn(K, C, 3, 3, device="cuda:0") * 0.2
    gy = torch.randn(N, K, H, W, device="cuda:0", dtype=DTYPE
                     ).contiguous(memory_format=torch.channels_last)
    by_in, by_out = x.numel() * 2, gy.numel() * 2
    with torch.no_grad():
        t_f = tm(lambda: conv3x3_reflect(x, w, None), reps)
        t_b = tm(lambda: conv3x3_bwd_data(gy, w), reps)
        extra = ""
        if args.miopen:
            xp = F.pad(x, (1, 1, 1, 1), mode="reflect")
            wb = w.to(DTYPE)
            t_mf = tm(lambda: F.conv2d(xp, wb), reps)
            extra = f" | miopen fwd {t_mf:7.3f}"
    rate_f = (by_in + by_out) / t_f / 1e9
    rate_b = (by_in + by_out) / t_b / 1e9
    # ceiling: the stream kernel on the larger of the two tensors
    ceil = bn_rate(max(by_in, by_out))
    print(f"{name:<16} {C:>3}->{K:<3} {H:>4}x{W:<4} | {t_f:7.3f} {rate_f:5.2f} "
          f"{ceil:5.2f} {100 * rate_f / ceil:4.0f} | {t_b:7.3f} {rate_b:5.2f} "
          f"{ceil:5.2f} {100 * rate_b / ceil:4.0f}{extra}")
    tot["fwd"] += t_f
    tot["bwd"] += t_b
    del x, gy
print(f"TOTAL fwd {tot['fwd']:.2f} ms  bwdD {tot['bwd']:.2f} ms "
      f"(wrapper time: weight pack + kernel(s) + fold)")
