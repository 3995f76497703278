"""Standalone timing of the fused BN kernels at the flagship shapes.

    python tools/bn_bench.py [--root OTHER_CHECKOUT] [--deterministic]
                             [--dtype {bf16,fp16}] [--encoder]

--root imports mine_amd from another built checkout, so two builds can be
timed with the same shape list. --deterministic runs the module in
deterministic mode (ops.backend) and times the order-fixed stats and
bwd_reduce launches next to the whole fwd+bwd. --encoder times the
encoder's small layers instead (batch 4, each with its own
activation, `res` for add_relu) and prints per-shape fwd+bwd DEVICE time
and the total weighted by how often the shape occurs in one step.
MINE_BN_COMPACT=0 keeps the small-layer path off.
"""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--deterministic", action="store_true")
ap.add_argument("--dtype", choices=("bf16", "fp16"), default="bf16")
ap.add_argument("--encoder", action="store_true")
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

# (N, C, H, W, act, layers per step): the 53 encoder layers
ENCODER = [
    (4, 64, 128, 192, "relu", 1),
    (4, 256, 64, 96, "none", 1), (4, 256, 64, 96, "add_relu", 3),
    (4, 512, 32, 48, "none", 1), (4, 512, 32, 48, "add_relu", 4),
    (4, 128, 64, 96, "relu", 1),
    (4, 64, 64, 96, "relu", 6),
    (4, 1024, 16, 24, "none", 1), (4, 1024, 16, 24, "add_relu", 6),
    (4, 256, 32, 48, "relu", 1),
    (4, 128, 32, 48, "relu", 7),
    (4, 2048, 8, 12, "none", 1), (4, 2048, 8, 12, "add_relu", 3),
    (4, 512, 16, 24, "relu", 1),
    (4, 256, 16, 24, "relu", 11),
    (4, 512, 8, 12, "relu", 5),
]


def device_ms(fn, n=20):
    """Device time of one call. The n calls are queued behind ~20 ms of
    matmul, so the host's launch cost is hidden and the two events bracket
    back-to-back kernels (launch gaps included)."""
    for _ in range(3):
        fn()
    a = torch.empty(8192, 8192, device="cuda:0")
    torch.cuda.synchronize()
    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for _ in range(3):
        a @ a
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def encoder():
    total = floor = 0.0
    for (N, C, H, W, act, count) in ENCODER:
        bn = FusedBNAct(C, act=act).cuda().train()
        cl = lambda t: t.contiguous(memory_format=torch.channels_last)
        x = cl(torch.randn(N, C, H, W, device="cuda:0", dtype=DTYPE)
               ).requires_grad_(True)
        res = cl(torch.randn_like(x)).requires_grad_(True) \
            if act == "add_relu" else None
        gy = cl(torch.randn_like(x))

        def step():
            y = bn(x, res) if res is not None else bn(x)
            y.backward(gy)
            x.grad = None
            if res is not None:
                res.grad = None

        t = device_ms(step)
        mb = N * C * H * W * 2 / 1e6
        # passes: stats 1r, fwd 1r1w, reduce 2r, dx 2r1w; add_relu reads
        # res three times and writes dres
        passes = 12 if act == "add_relu" else 8
        print(f"N{N} C{C} {H}x{W} {act:8s} x{count:2d}: fwd+bwd {t*1000:7.1f} us"
              f"  tensor {mb:5.1f} MB  -> {mb*passes/t/1000:5.2f} TB/s")
        total += count * t
        floor += count * mb * passes / 6.3e3
    print(f"WEIGHTED TOTAL {total:.3f} ms per step over "
          f"{sum(e[5] for e in ENCODER)} layers; traffic floor at 6.3 TB/s "
          f"{floor:.3f} ms")


ext = get_extension(required=True)
if args.encoder:
    print("encoder shapes, dtype:", args.dtype, " compact:",
          os.environ.get("MINE_BN_COMPACT", "1"))
    encoder()
    sys.exit(0)
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
