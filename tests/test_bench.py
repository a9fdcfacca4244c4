# Copyright (c) Flashy-AMD authors.
"""bench.py command-line contract on the CPU path: a plain run times exactly
--steps steps and measures nothing else, --full adds the checkpoint figures,
--dump-outputs writes one step from the seeded start, reproducibly."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


def _bench(*args: str, cwd: Path) -> dict:
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env["CUDA_VISIBLE_DEVICES"] = ""   # the CPU path, also on a GPU machine
    env["HIP_VISIBLE_DEVICES"] = ""
    out = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--batch", "4", *args],
        cwd=cwd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def _load(folder: Path) -> dict:
    return {p.name: np.load(p) for p in sorted(folder.glob("*.npy"))}


def test_plain_run_dumps_reproducible_outputs(tmp_path):
    res = _bench("--dump-outputs", str(tmp_path / "a"), cwd=tmp_path)
    assert res["steps"] == 2 and res["warmup"] == 1
    assert res["metric"] == "img/sec" and res["unit"] == "img/s"
    assert res["higher_is_better"] is True
    assert res["ms_per_step"] > 0
    # value and ms_per_step describe the same 2 timed steps of batch 4
    assert abs(res["value"] * res["ms_per_step"] / 1000 - 4) < 1e-6
    # a plain run measures nothing but the step
    assert res["config"]["checkpoint_save_s"] is None
    assert res["config"]["large_checkpoint"] is None

    a = _load(tmp_path / "a")
    assert "loss.npy" in a and "model.fc.weight.npy" in a
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.isfinite(a["loss.npy"]).all()

    _bench("--dump-outputs", str(tmp_path / "b"), cwd=tmp_path)
    b = _load(tmp_path / "b")
    assert a.keys() == b.keys()
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)

    # the dumped step starts from the seeded state, whatever was timed
    res = _bench("--steps", "3", "--dump-outputs", str(tmp_path / "c"),
                 cwd=tmp_path)
    assert res["steps"] == 3
    c = _load(tmp_path / "c")
    for name in a:
        np.testing.assert_array_equal(a[name], c[name], err_msg=name)
    # ... and is a real training step: weights moved off their init
    import torch
    from flashy_amd.models import resnet18
    torch.manual_seed(1234)
    init = resnet18(num_classes=10, small_input=True).fc.weight.detach().numpy()
    assert a["model.fc.weight.npy"].shape == init.shape
    assert 0 < np.abs(a["model.fc.weight.npy"] - init).max() < 1.0


def test_full_run_adds_checkpoint_figures(tmp_path):
    res = _bench("--full", cwd=tmp_path)
    assert res["steps"] == 2
    assert res["config"]["checkpoint_save_s"] > 0
    assert res["config"]["checkpoint_restore_s"] > 0
    assert not list(tmp_path.iterdir())   # the round-trip file is removed


def test_dump_outputs_samples_large_state(tmp_path, monkeypatch):
    """State above the budget is cut to a fixed sample: same entries on
    every call, each tensor shrunk by the same factor."""
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    torch.manual_seed(0)
    net = torch.nn.Linear(100, 40)            # 4040 floats = 16160 bytes
    loss = torch.tensor(1.5)
    bench.dump_outputs(str(tmp_path / "a"), loss, {"net": net})
    bench.dump_outputs(str(tmp_path / "b"), loss, {"net": net})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["loss.npy", "net.bias.npy", "net.weight.npy"]
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert a["loss.npy"] == np.float32(1.5)
    w = a["net.weight.npy"]
    assert w.ndim == 1 and 0 < w.size < 4000
    assert np.isin(w, net.weight.detach().numpy()).all()
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
