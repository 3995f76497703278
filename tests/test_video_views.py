"""The video tool renders its trajectory `views` poses per launch: the
frames it writes must not depend on that number. Five frames with
views=4 make one full chunk and one partial chunk (a single frame, which
takes the single-view op). Runs on the GPU when there is one, else on the
CPU path."""
import os

import numpy as np
import torch

from mine_amd.config import RuntimeState, default_config
from mine_amd.engine import SynthesisTask


def _frames(out_dir):
    from PIL import Image
    fdir = os.path.join(out_dir, "frames")
    names = sorted(n for n in os.listdir(fdir) if n.endswith(".png"))
    return names, [np.asarray(Image.open(os.path.join(fdir, n))) for n in names]


def test_chunked_video_frames_equal_per_frame_loop(tmp_path, monkeypatch):
    from visualizations.image_to_video import (VideoGenerator,
                                               load_source_image,
                                               path_planning)
    monkeypatch.setattr(VideoGenerator, "_encode",
                        staticmethod(lambda *a, **k: None))   # no ffmpeg run
    dev = "cuda:0" if torch.cuda.is_available() else "cpu"
    H, W = 32, 48
    cfg = default_config(**{
        "data.name": "realestate10k", "data.img_h": H, "data.img_w": W,
        "mpi.num_bins_coarse": 4, "data.per_gpu_batch_size": 1,
        "data.visible_point_count": 8, "training.amp_dtype": "fp32"})
    torch.manual_seed(3)
    task = SynthesisTask(cfg, state=RuntimeState(), is_val=True, device=dev)
    gen = VideoGenerator(task, cfg, torch.device(dev))
    gen.infer_mpi(load_source_image(None, H, W))
    offsets = path_planning("circle", 0.06, 0.03, 0.12, 5)

    calls = []
    real = gen.render_poses
    monkeypatch.setattr(gen, "render_poses",
                        lambda offs: calls.append(len(offs)) or real(offs))
    one, four = str(tmp_path / "v1"), str(tmp_path / "v4")
    gen.render_video(offsets, one, save_depth=True, views=1)
    assert calls == []
    gen.render_video(offsets, four, save_depth=True, views=4)
    assert calls == [4, 1]

    names1, frames1 = _frames(one)
    names4, frames4 = _frames(four)
    assert names1 == names4 and len(names1) == 10     # rgb + disparity
    for n, a, b in zip(names1, frames1, frames4):
        assert a.shape == (H, W, 3) and a.dtype == np.uint8
        assert np.array_equal(a, b), n
    assert not np.array_equal(frames1[1], frames1[2])  # the camera moves
    # the chunked benchmark path runs and reports a rate
    assert gen.benchmark_fps(offsets, warmup=1, views=4) > 0
