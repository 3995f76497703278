"""Deterministic mode, public surface (CPU): the config key, the
set/is/context-manager trio in ops.backend, the MINE_DETERMINISTIC
environment variable and SynthesisTask's wiring of the key."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def restore_mode():
    """Leave the process-wide mode as the test found it."""
    from mine_amd.ops import backend
    prev = backend._DETERMINISTIC
    yield
    backend._DETERMINISTIC = prev


def test_config_key():
    from mine_amd.config import default_config
    assert default_config()["training.deterministic"] is False
    cfg = default_config(**{"training.deterministic": True})
    assert cfg["training.deterministic"] is True


def test_reexported_from_ops():
    import mine_amd.ops as ops
    from mine_amd.ops import backend
    assert ops.set_deterministic is backend.set_deterministic
    assert ops.is_deterministic is backend.is_deterministic
    assert ops.deterministic is backend.deterministic


def test_set_and_context_manager(restore_mode):
    from mine_amd.ops import deterministic, is_deterministic, \
        set_deterministic

    set_deterministic(False)
    assert is_deterministic() is False
    with deterministic():
        assert is_deterministic() is True
        with deterministic(False):
            assert is_deterministic() is False
            with deterministic(True):
                assert is_deterministic() is True
            assert is_deterministic() is False
        assert is_deterministic() is True
    assert is_deterministic() is False

    set_deterministic(True)
    with deterministic(False):
        assert is_deterministic() is False
    assert is_deterministic() is True

    # restored when the body raises
    set_deterministic(False)
    with pytest.raises(ValueError):
        with deterministic():
            assert is_deterministic() is True
            raise ValueError("body failed")
    assert is_deterministic() is False


@pytest.mark.parametrize("value,expected", [("1", "True"), ("0", "False"),
                                            (None, "False")])
def test_environment_variable(value, expected):
    env = dict(os.environ)
    env.pop("MINE_DETERMINISTIC", None)
    if value is not None:
        env["MINE_DETERMINISTIC"] = value
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-c",
         "import mine_amd.ops as o; print(o.is_deterministic())"],
        env=env, cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == expected


def test_task_sets_mode(tiny_config, restore_mode):
    import torch
    from mine_amd.data import SyntheticMPIDataset, collate_src_tgt
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import is_deterministic, set_deterministic
    from mine_amd.ops import conv

    set_deterministic(False)
    prev_cudnn = torch.backends.cudnn.deterministic
    prev_force = conv._FORCE_IGEMM
    try:
        cfg = tiny_config.replace(**{"training.deterministic": True})
        task = SynthesisTask(cfg, device="cpu")
        ds = SyntheticMPIDataset(cfg, length=2)
        loss_dict = task.train_step(collate_src_tgt([ds[i] for i in range(2)]))
        loss = float(loss_dict["loss"])
        assert loss == loss and loss > 0
        assert is_deterministic() is True
        assert conv._FORCE_IGEMM is True
        assert torch.backends.cudnn.deterministic is True
    finally:
        torch.backends.cudnn.deterministic = prev_cudnn
        conv.set_force_igemm(prev_force)


def test_task_leaves_mode_alone_when_key_is_false(tiny_config, restore_mode):
    from mine_amd.engine import SynthesisTask
    from mine_amd.ops import is_deterministic, set_deterministic

    set_deterministic(True)  # as MINE_DETERMINISTIC=1 would
    SynthesisTask(tiny_config, device="cpu")
    assert is_deterministic() is True
