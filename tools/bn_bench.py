"""Standalone timing of the fused BN kernels at the flagship shapes.

    python tools/bn_bench.py [--root OTHER_CHECKOUT] [--deterministic]
                             [--dtype {bf16,fp16}]

--root imports mine_amd from another built checkout, so two builds can be
timed with the same shape list. --deterministic runs the module in
deterministic mode (ops.backend) and times the order-fixed stats and
bwd_reduce launches next to the whole fwd+bwd.
"""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--deterministic", action="store_true")
ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
args = ap.parse_args()
sys.path.insert(0, args.root)
import torch
from mine_amd.ops.backend import get_extension
from mine_amd.ops.bn import FusedBNAct, _ACT

DTYPE = torch.float16 if args.dtype == "fp16" else torch.bfloat16

if args.deterministic:
    from mine_amd.ops.backend import set_deterministic
    set_deterministic(True)
# trailing argument of the reduction bindings; older checkouts lack it
DET = (True,) if args.deterministic else ()

SHAPES = [  # (N, C, H, W) decoder's big BN layers + one encoder-ish
    (256, 16, 256, 384),
    (256, 32, 128, 192),
    (256, 16, 128, 192),
    (256, 64, 64, 96),
    (256, 128, 32, 48),
    (256, 64, 32, 48),
    (256, 256, 16, 24),
    (4, 64, 128, 192),
    (4, 256, 64, 96),
]

def tm(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1000

ext = get_extension(required=True)
print("mode:", "deterministic" if args.deterministic else "default",
      " dtype:", args.dtype)
tot = tot_s = tot_r = 0.0
for (N, C, H, W) in SHAPES:
    bn = FusedBNAct(C, act="elu").cuda().train()
    x = torch.randn(N, C, H, W, device="cuda:0", dtype=DTYPE
                    ).contiguous(memory_format=torch.channels_last
                    ).requires_grad_(True)
    gy = torch.randn_like(x)

    def step():
        y = bn(x)
        y.backward(gy)
        x.grad = None

    # the two reductions alone, through the bindings the module uses
    M = N * H * W
    xf = x.detach().permute(0, 2, 3, 1).reshape(-1)
    gf = gy.permute(0, 2, 3, 1).reshape(-1)
    none = torch.empty(0, device="cuda:0", dtype=DTYPE)
    rm, rv = torch.zeros(C, device="cuda:0"), torch.ones(C, device="cuda:0")
    ga, be = bn.weight.detach().float(), bn.bias.detach().float()
    mean, invstd = ext.bn_stats(xf, M, C, rm, rv, 1e-5, 0.1, 0, *DET)

    def stats():
        ext.bn_stats(xf, M, C, rm, rv, 1e-5, 0.1, 0, *DET)

    def reduce():
        ext.bn_act_bwd_reduce(xf, none, gf, mean, invstd, ga, be, M, C,
                              _ACT["elu"], 0, *DET)

    t, ts, tr = tm(step), tm(stats), tm(reduce)
    gb = N * C * H * W * 2 / 1e9
    # stats(1r) + fwd(1r1w) + reduce(2r) + dx(2r1w) = 6r + 2w = 8 passes
    print(f"N{N} C{C} {H}x{W}: fwd+bwd {t:7.3f} ms  tensor {gb*1000:.0f} MB"
          f"  -> {gb*8/t*1000:.0f} GB/s of {6300}"
          f"  | stats {ts:6.3f} ms ({gb/ts*1000:.0f} GB/s)"
          f"  bwd_reduce {tr:6.3f} ms ({gb*2/tr*1000:.0f} GB/s)")
    tot += t
    tot_s += ts
    tot_r += tr
print(f"TOTAL {tot:.2f} ms  stats {tot_s:.2f} ms  bwd_reduce {tot_r:.2f} ms")
