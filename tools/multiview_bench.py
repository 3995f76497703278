"""Train-step time and peak memory with several target views per sample.

    python tools/multiview_bench.py [--views 2] [--steps 12] [--warmup 4]
                                    [--rounds 3] [--batch 4] [--planes 64]
                                    [--height 256] [--width 384]

Three cases on one model and one batch, at the flagship shapes by default:

  L=1        one target view: the single-view op, as before
  L=V        V target views through render_tgt_views (one MPI, one
             MPI-sized gradient buffer)
  L=V copy   V target views on the single-view op, the way a caller had to
             write it before: the blended MPI repeated V times
             (`expand(...).contiguous()`) at every scale, and autograd
             summing the V slices of the V-times-larger gradient

The cases are timed alternately, `--rounds` times, so that a drift of the
machine shows as a spread within a case; a round is `--steps` eager train
steps between two device synchronisations after `--warmup` steps. Peak
memory is torch.cuda.max_memory_allocated over the timed steps of a round.
Prints one JSON line per case and round, then one summary line per case
(median ms, min..max, peak MiB).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=2)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=384)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no CPU fall-back"

    from mine_amd.config import default_config
    from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import render_tgt_view

    V = args.views
    over = {"data.name": "realestate10k", "data.img_h": args.height,
            "data.img_w": args.width, "mpi.num_bins_coarse": args.planes,
            "data.per_gpu_batch_size": args.batch,
            "data.visible_point_count": 256, "data.num_tgt_views": V}
    cfg = default_config(**over)
    ds = SyntheticMPIDataset(cfg, length=args.batch)
    src, tgt = collate_src_tgt([ds[i] for i in range(args.batch)])
    items_v = (src, tgt)
    items_1 = (src, {k: v[:, :1].contiguous() for k, v in tgt.items()})

    torch.manual_seed(0)
    task = SynthesisTask(cfg, device="cuda:0")
    plain = task.render_novel_view

    def copy_render(mpi, disparity, G_tgt_src, K_src_inv, K_tgt,
                    scale_factor=None):
        """render_novel_view on the single-view op with a repeated MPI."""
        B = mpi.shape[0]
        n = G_tgt_src.shape[0] // B
        if scale_factor is not None:
            with torch.no_grad():
                G_tgt_src = G_tgt_src.clone()
                G_tgt_src[:, 0:3, 3] /= scale_factor.repeat(n).view(-1, 1)
        big = mpi.unsqueeze(0).expand(n, *mpi.shape) \
            .reshape(n * B, *mpi.shape[1:]).contiguous()
        rgb, depth, mask = render_tgt_view(
            big, disparity.repeat(n, 1), G_tgt_src, K_src_inv.repeat(n, 1, 1),
            K_tgt, bg_depth_inf=task.bg_depth_inf, use_alpha=task.use_alpha)
        return {"tgt_imgs_syn": rgb,
                "tgt_disparity_syn": torch.reciprocal(depth),
                "tgt_mask_syn": mask}

    cases = [("L=1", items_1, plain), (f"L={V}", items_v, plain),
             (f"L={V} copy", items_v, copy_render)]

    def steps(items, render, n):
        task.render_novel_view = render
        for _ in range(n):
            task.global_step += 1      # monitors off except on logging steps
            task.train_step(items)
        torch.cuda.synchronize()

    for _, items, render in cases:
        steps(items, render, args.warmup)
    rows = {name: [] for name, _, _ in cases}
    for rnd in range(args.rounds):
        for name, items, render in cases:
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            steps(items, render, args.steps)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            peak = torch.cuda.max_memory_allocated() / 2 ** 20
            rows[name].append((ms, peak))
            print(json.dumps({"case": name, "round": rnd,
                              "ms_per_step": round(ms, 2),
                              "peak_mib": round(peak, 1)}), flush=True)
    for name, r in rows.items():
        ms = [a for a, _ in r]
        print(f"{name:<10} median {statistics.median(ms):8.2f} ms/step "
              f"({min(ms):.2f}..{max(ms):.2f}), peak "
              f"{max(p for _, p in r):9.1f} MiB")
    return 0


if __name__ == "__main__":
    sys.exit(main())
