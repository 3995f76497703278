#!/usr/bin/env python3
"""Flagship training benchmark — RealEstate10K 384x256 N=64, bf16, DDP.

Measures the BASELINE.json headline metric: train imgs/sec (whole job)
on the reference's flagship config (384x256, 64 planes, per-GPU batch 4,
ref configs/params_realestate.yaml) with synthetic data of that shape and
random-init weights (no network access in this environment).

    python bench.py --gpus 1 --steps 30 --warmup 10
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 \
        --master-addr 127.0.0.1 bench.py --gpus 8 --steps 30 --warmup 10

One rank per GPU over RCCL; rank 0 prints ONE JSON line.

A plain run sets up, warms up, times --steps train steps and prints the
result line. --full adds the measurements the headline figure does not
need (the multi-GPU 64 MiB all-reduce bandwidth probe). --dump-outputs
DIR writes what one step of the timed path returns, its loss dict, as
DIR/<name>.npy; together with --full it adds a seeded sample of that
step's gradients and updated parameters (not reproducible on the GPU, see
step_outputs). Model init, disparity sampling and data are seeded. The
timed loop is the same with and without the option; the dumped step is
run once more after the clock has stopped, from the seeded weights and a
fresh Adam state on the last timed step's batch, so two builds run with
the same arguments see identical inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


DUMP_BYTE_LIMIT = 64 << 20


def snapshot_state(task):
    """Copies of the seeded parameters and buffers, for restore_state()."""
    live = [t for m in (task.backbone, task.decoder)
            for t in list(m.parameters()) + list(m.buffers())]
    return live, [t.detach().clone() for t in live]


def restore_state(task, snap) -> None:
    """Put the model back to its seeded weights and Adam back to step 0,
    all in place (the tensors keep their addresses, so a captured graph
    and the gradient buckets stay valid)."""
    import torch

    live, saved = snap
    with torch.no_grad():
        for t, s in zip(live, saved):
            t.copy_(s)
        for st in task.optimizer.state.values():
            for v in st.values():
                if torch.is_tensor(v):
                    v.zero_()


SAMPLE_ELEMS = 1 << 20


def step_outputs(task, loss_dict: dict, with_state: bool) -> dict:
    """What one train step produced: the loss dict it returned and, with
    with_state, a fixed seeded sample (SAMPLE_ELEMS elements each, drawn
    over all parameters in optimizer order) of the reduced gradients it
    left in .grad and of the parameters after its Adam update.

    The samples sit behind --full because on the GPU they are not
    reproducible: BatchNorm statistics are summed with fp32 atomics, the
    random-init bf16 network amplifies that to bf16-epsilon differences on
    most output elements, and the gradients of two identical steps then
    differ by about their own norm (docs/NEXT.md section 7). The loss
    terms, being means, agree to 1e-4 or better."""
    import torch

    out = {k: v for k, v in loss_dict.items() if torch.is_tensor(v)}
    if not with_state:
        return out
    params = [p for g in task.optimizer.param_groups for p in g["params"]
              if p.grad is not None]
    with torch.no_grad():
        grads = torch.cat([p.grad.reshape(-1).float() for p in params])
        after = torch.cat([p.reshape(-1).float() for p in params])
        idx = torch.randint(grads.numel(), (SAMPLE_ELEMS,),
                            generator=torch.Generator().manual_seed(0))
        idx = idx.sort().values.to(grads.device)
        out["grad_sample"] = grads[idx]
        out["param_sample"] = after[idx]
    return out


def dump_outputs(out_dir: str, outputs: dict) -> None:
    """Write each tensor as <out_dir>/<name>.npy, float32."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in outputs.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        total += a.nbytes
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    assert total <= DUMP_BYTE_LIMIT, total


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--batch", type=int, default=4, help="per-GPU batch size")
    p.add_argument("--planes", type=int, default=64)
    p.add_argument("--height", type=int, default=256)
    p.add_argument("--width", type=int, default=384)
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--dataset", type=str, default="realestate10k")
    p.add_argument("--graph", action="store_true",
                   help="try the hipGraph-captured train step (capture "
                        "falls back to eager; currently blocked by the "
                        "three remaining library convs allocating "
                        "workspace mid-capture — docs/NEXT.md)")
    p.add_argument("--timers", action="store_true",
                   help="print a sync-bracketed per-phase breakdown (diagnostic "
                        "run only; the extra syncs perturb the headline number)")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements the headline figure "
                        "does not need (multi-GPU: 64 MiB all-reduce "
                        "bus-bandwidth probe; with --dump-outputs: gradient "
                        "and updated-parameter samples)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, run the timed path once "
                        "more from the seeded weights and write its loss "
                        "dict as DIR/<name>.npy (fp32)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")

    import torch
    import torch.distributed as dist

    from mine_amd.config import RuntimeState, default_config
    from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
    from mine_amd.engine import SynthesisTask
    from mine_amd.parallel import init_distributed

    rank, local_rank, world_size = init_distributed()
    if world_size > 1:
        assert world_size == args.gpus, (world_size, args.gpus)
    use_gpu = torch.cuda.is_available()
    if use_gpu:
        torch.cuda.set_device(local_rank % torch.cuda.device_count())
    device = f"cuda:{local_rank % torch.cuda.device_count()}" if use_gpu else "cpu"

    if world_size > 1:
        # RCCL self-check BEFORE any model work (VERDICT round-1 item 6):
        # a known-value all-reduce proves the collective path.
        comm_dev = device if dist.get_backend() == "nccl" else "cpu"
        probe = torch.full((1,), float(rank + 1), device=comm_dev)
        dist.all_reduce(probe)
        expect = world_size * (world_size + 1) / 2
        assert abs(float(probe.item()) - expect) < 1e-3, \
            f"all-reduce self-check failed: {probe.item()} != {expect}"

    if world_size > 1 and args.full:
        # --full: a 64 MiB ring probe prints the achieved bus bandwidth
        # so a multi-GPU run yields a diagnosable number.
        big = torch.ones(16 << 20, device=comm_dev)  # 64 MiB fp32
        for _ in range(2):
            dist.all_reduce(big)
        if use_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            dist.all_reduce(big)
        if use_gpu:
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 4
        # ring all-reduce moves 2*(n-1)/n of the payload per link
        busbw = (big.numel() * 4 / dt) * 2 * (world_size - 1) / world_size / 1e9
        if rank == 0:
            print(json.dumps({"rccl_selfcheck": "ok",
                              "allreduce_64MiB_ms": round(dt * 1e3, 2),
                              "busbw_GBps": round(busbw, 1)}),
                  file=sys.stderr)

    cfg = default_config(**{
        "data.name": args.dataset,
        "data.img_h": args.height, "data.img_w": args.width,
        "mpi.num_bins_coarse": args.planes,
        "data.per_gpu_batch_size": args.batch,
        "data.visible_point_count": 256,
        "lr.backbone_lr": 0.0002, "lr.decay_steps": [4, 8],
        "training.amp_dtype": args.dtype,
        # no logging happens in a bench run: keep the monitor-only loss
        # terms (src L1/SSIM/smooth, PSNR) out of the timed region
        "training.log_interval": 1 << 30,
    })
    state = RuntimeState(global_rank=rank, local_rank=local_rank,
                         world_size=world_size)
    # Fixed seed (host and device generators): the random-init weights and
    # the per-step disparity samples are the same in every run, so
    # --dump-outputs of two builds can be compared output for output.
    torch.manual_seed(20210829)
    task = SynthesisTask(cfg, state=state)
    seeded = snapshot_state(task) if args.dump_outputs else None
    # identical weights on every rank, distinct disparity samples per rank
    torch.manual_seed(20210829 + 1 + rank)

    # Pre-build a few host-side batches; the H2D staging stays inside the
    # timed region (it is part of a real training step). Each rank gets
    # DISTINCT data (per-rank seed) so the gradient all-reduce moves
    # real information, as in training.
    ds = SyntheticMPIDataset(cfg, length=args.batch * 4)
    ds.seed_base = 1 + rank
    batches = [collate_src_tgt([ds[i * args.batch + j] for j in range(args.batch)])
               for i in range(4)]

    def sync():
        if use_gpu:
            torch.cuda.synchronize()
        if world_size > 1:
            dist.barrier()
            if use_gpu:
                torch.cuda.synchronize()

    graphed = False
    if use_gpu and world_size == 1 and args.dtype != "fp16" and \
            args.graph and not args.timers:
        graphed = task.enable_graph_step(batches[0])
        if rank == 0:
            print(json.dumps({"hip_graph_step": bool(graphed)}),
                  file=sys.stderr)
    step_fn = task.train_step_graphed if graphed else task.train_step

    for i in range(args.warmup):
        step_fn(batches[i % len(batches)])

    if args.timers:
        task.enable_phase_timers()
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step_fn(batches[i % len(batches)])
    sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        # The kernels accumulate with fp32 atomics and Adam turns that
        # rounding noise into full-size weight updates, so after a few
        # steps two runs hold visibly different weights. The dump therefore
        # comes from one more step of the timed path, run after the clock
        # has stopped, from the seeded weights and a zeroed Adam state on
        # the last timed step's batch: it depends on the arguments alone.
        # Every rank takes part (the step all-reduces); rank 0 writes.
        restore_state(task, seeded)
        torch.manual_seed(20210829 + 1 + rank)
        outputs = step_outputs(
            task, step_fn(batches[(args.steps - 1) % len(batches)]),
            with_state=args.full)
        sync()
        if rank == 0:
            dump_outputs(args.dump_outputs, outputs)

    # MAX elapsed over ranks = whole-job wall time
    if world_size > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device=device if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    imgs_per_sec = world_size * args.batch * args.steps / elapsed
    if args.timers and rank == 0:
        phases = {k: round(v * 1000.0, 1)
                  for k, v in task.pop_phase_times().items()}
        print(json.dumps({"phase_ms": phases}), file=sys.stderr)
    if rank == 0:
        metric = "train imgs/sec (whole node) RealEstate10K 384x256 N=64"
        if (args.dataset, args.height, args.width, args.planes) != \
                ("realestate10k", 256, 384, 64):
            metric = (f"train imgs/sec (whole node) {args.dataset} "
                      f"{args.width}x{args.height} N={args.planes}")
        result = {
            "metric": metric,
            "value": round(imgs_per_sec, 3),
            "unit": "imgs/sec",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1000.0, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": "monodepth2-resnet50-mpi",
                "global_batch": world_size * args.batch,
                "seq_len": args.planes,
                "parallelism": f"dp{world_size}",
                "img_h": args.height,
                "img_w": args.width,
                "n_planes": args.planes,
            },
        }
        print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
