"""mine_amd — MI355X-native continuous-depth-MPI framework.

A from-scratch implementation of the capabilities of vincentfung13/MINE
("MINE: Towards Continuous Depth MPI with NeRF for Novel View Synthesis",
ICCV 2021), designed MI355X-first:

  * PyTorch-ROCm frontend (autograd, optimizer, data loading)
  * hand-written HIP/CDNA4 kernels (gfx950) for the hot rendering path:
    fused plane-sweep homography warp + z-cull + over-composite across all
    N depth planes, fused src-view volume compositing with RGB blending,
    fused SSIM — no per-plane intermediates are ever materialized
  * RCCL over xGMI for data-parallel training (own bucketed gradient
    all-reduce engine overlapped with backward)

Layer map mirrors SURVEY.md section 1 of the reference analysis:
  config   — mine_amd.config        (ref: train.py:30-56)
  engine   — mine_amd.engine        (ref: synthesis_task.py)
  models   — mine_amd.models        (ref: network/)
  ops      — mine_amd.ops           (ref: operations/)
  data     — mine_amd.data          (ref: input_pipelines/)
  parallel — mine_amd.parallel      (ref: DDP/SyncBN usage)
  utils    — mine_amd.utils
"""

__version__ = "0.1.0"

import os as _os

# MIOpen solver selection. Measured on MI355X at the flagship config
# (384x256 N=64 B=4 bf16): FAST's heuristic picks zero-workspace naive
# fallback kernels for the backward-data/backward-weight convs and the
# step runs 5.0 s (backward alone 4.84 s); DYNAMIC_HYBRID finds tuned
# implicit-GEMM MFMA solvers and the same step runs 0.29 s — 17x. So:
# DYNAMIC_HYBRID, with the find results shipped in-tree
# (mine_amd/miopen_db) so a fresh box skips the ~60 s one-time find.
# Both knobs respect pre-set environment overrides.
#
# MIOpen appends every new find result to its user db and rewrites the
# files in place, so it is never pointed at the tracked files: they seed
# a per-user copy (keyed by their content, so an updated in-tree db
# starts a fresh copy) and MIOpen reads and writes that.


def _seed_user_db(src_dir: str) -> str:
    import hashlib
    import shutil
    import tempfile

    names = sorted(n for n in _os.listdir(src_dir) if n.endswith(".txt"))
    h = hashlib.sha1()
    for n in names:
        with open(_os.path.join(src_dir, n), "rb") as f:
            h.update(n.encode() + b"\0" + f.read())
    sub = _os.path.join("mine_amd", "miopen_db-" + h.hexdigest()[:12])
    cache = _os.environ.get("XDG_CACHE_HOME") or \
        _os.path.join(_os.path.expanduser("~"), ".cache")
    for base in (cache, _os.path.join(tempfile.gettempdir(),
                                      f"mine_amd-{_os.getuid()}")):
        dst_dir = _os.path.join(base, sub)
        try:
            _os.makedirs(dst_dir, exist_ok=True)
            for n in names:
                dst = _os.path.join(dst_dir, n)
                if not _os.path.exists(dst):
                    # copy-then-rename: ranks starting together never
                    # see a half-written db
                    tmp = f"{dst}.{_os.getpid()}.tmp"
                    shutil.copyfile(_os.path.join(src_dir, n), tmp)
                    _os.replace(tmp, dst)
            return dst_dir
        except OSError:
            continue
    return None  # nowhere to copy to: MIOpen keeps its own default user db


_os.environ.setdefault("MIOPEN_FIND_MODE", "DYNAMIC_HYBRID")
_db_dir = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "miopen_db")
if _os.path.isdir(_db_dir) and "MIOPEN_USER_DB_PATH" not in _os.environ:
    _user_db = _seed_user_db(_db_dir)
    if _user_db is not None:
        _os.environ["MIOPEN_USER_DB_PATH"] = _user_db

from mine_amd.config import Config, load_config  # noqa: F401
