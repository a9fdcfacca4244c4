# Copyright (c) Flashy-AMD authors.
"""CPU tests of flashy_amd.data.DeviceAugment: the counter hash (pinned
against literal values and checked for uniformity), the crop / flip / pad
geometry of the torch path against an independent pad-and-slice
construction, state round trips, argument validation, and the CIFAR example
with ``augment.enabled=true`` through the real CLI."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from torch.nn import functional as F

from flashy_amd.data import DeviceAugment

REPO = Path(__file__).resolve().parent.parent

CIFAR = dict(mean=(0.4914, 0.4822, 0.4465), std=(0.2023, 0.1994, 0.2010))


def _aug(out_size, **kw):
    kw.setdefault("device", "cpu")
    return DeviceAugment(out_size, **kw)


def _batch(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


# -- the hash ---------------------------------------------------------------

# (seed, step, ny, nx, p_flip) -> (dy, dx, flip) of samples 0..3, computed
# once from the pseudocode in docs/kernels.md by a stand-alone snippet
HASH_TABLE = [
    ((0, 0, 9, 9, 0.5),
     [(2, 5, True), (8, 6, True), (8, 3, True), (4, 5, False)]),
    ((0, 1, 9, 9, 0.5),
     [(8, 2, False), (2, 1, False), (7, 7, True), (3, 1, False)]),
    ((1234, 7, 33, 33, 0.5),
     [(8, 4, True), (29, 21, True), (13, 29, True), (3, 13, False)]),
    ((1234, 1000, 5, 3, 0.25),
     [(2, 1, False), (1, 0, False), (1, 2, False), (0, 0, True)]),
    ((2 ** 63 + 5, 2 ** 40, 9, 33, 0.5),
     [(1, 0, True), (3, 7, True), (0, 15, True), (7, 27, False)]),
]


@pytest.mark.parametrize("key,want", HASH_TABLE)
def test_params_at_literal_table(key, want):
    seed, step, ny, nx, p = key
    aug = _aug(8, flip=p, seed=seed)
    dy, dx, flip = aug.params_at(step, 4, (8 + ny - 1, 8 + nx - 1))
    assert dy.dtype == dx.dtype == torch.int64 and flip.dtype == torch.bool
    got = list(zip(dy.tolist(), dx.tolist(), flip.tolist()))
    assert got == want


@pytest.mark.parametrize("seed", [0, 1234])
@pytest.mark.parametrize("rng", [9, 33])
def test_hash_uniformity(seed, rng):
    """65,536 draws (steps 0..1023 x samples 0..63): every offset value's
    count and the flip count lie within 5 binomial standard deviations."""
    aug = _aug(8, seed=seed)
    size = (8 + rng - 1, 8 + rng - 1)
    draws = [aug.params_at(step, 64, size) for step in range(1024)]
    dy = torch.cat([d[0] for d in draws])
    dx = torch.cat([d[1] for d in draws])
    flip = torch.cat([d[2] for d in draws])
    n = dy.numel()
    assert n == 65536
    p = 1.0 / rng
    sd = math.sqrt(n * p * (1 - p))
    for name, v in (("dy", dy), ("dx", dx)):
        assert 0 <= int(v.min()) and int(v.max()) == rng - 1
        counts = torch.bincount(v, minlength=rng).double()
        worst = float((counts - n * p).abs().max()) / sd
        print(f"seed {seed} range {rng} {name}: worst {worst:.2f} sd")
        assert worst <= 5.0, (name, worst)
    z = abs(int(flip.sum()) - n / 2) / math.sqrt(n / 4)
    print(f"seed {seed} range {rng} flip: {z:.2f} sd")
    assert z <= 5.0, z


def test_scale_bias_are_fp32_of_the_double_values():
    aug = _aug(32, **CIFAR)
    for c in range(3):
        assert aug.scale[c] == float(np.float32(1.0 / (255.0 * CIFAR["std"][c])))
        assert aug.bias[c] == float(
            np.float32(-CIFAR["mean"][c] / CIFAR["std"][c]))


# -- geometry ---------------------------------------------------------------

def _independent(aug, src, step, train=True):
    """pad the batch, slice each sample at its offsets, flip, normalize."""
    n, h, w, _ = src.shape
    oh, ow = aug.out_size
    p = aug.pad
    padded = F.pad(src.permute(0, 3, 1, 2), (p, p, p, p), value=aug.fill)
    padded = padded.permute(0, 2, 3, 1)
    if train:
        dy, dx, flip = aug.params_at(step, n, (h, w))
    else:
        dy = torch.full((n,), (h + 2 * p - oh) // 2)
        dx = torch.full((n,), (w + 2 * p - ow) // 2)
        flip = torch.zeros(n, dtype=torch.bool)
    rows = []
    for i in range(n):
        crop = padded[i, int(dy[i]):int(dy[i]) + oh, int(dx[i]):int(dx[i]) + ow]
        rows.append(crop.flip(-2) if flip[i] else crop)
    crop = torch.stack(rows).double()
    scale = torch.tensor(aug.scale, dtype=torch.float64)
    bias = torch.tensor(aug.bias, dtype=torch.float64)
    return (crop * scale + bias).float().bfloat16()


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


GEOMETRY = [
    # n, (h, w), out, kwargs
    (5, (8, 8), 8, dict(pad=2)),
    (3, (10, 12), 8, dict(pad=0)),
    (4, (9, 9), (6, 7), dict(pad=1)),
    (5, (8, 8), 8, dict(pad=2, fill=7, **CIFAR)),
    (6, (8, 8), 8, dict(pad=2, flip=0.0)),
    (6, (8, 8), 8, dict(pad=2, flip=1.0, **CIFAR)),
]


@pytest.mark.parametrize("n,size,out,kw", GEOMETRY)
def test_geometry_matches_pad_and_slice(n, size, out, kw):
    aug = _aug(out, seed=11, **kw)
    ref = _aug(out, seed=11, **kw)
    for step in range(3):
        src = _batch(n, *size, seed=step)
        got = aug(src)
        assert got.dtype == torch.bfloat16
        assert tuple(got.shape) == (n, *aug.out_size, 3)
        assert _same(got, _independent(ref, src, step))
    assert aug.state_dict() == {"seed": 11, "step": 3}
    if "flip" in kw:
        flips = ref.params_at(0, n, size)[2]
        assert bool(flips.all()) == (kw["flip"] == 1.0)
        assert bool(flips.any()) == (kw["flip"] == 1.0)


def test_padding_and_flip_actually_occur():
    """The pad case draws offsets that reach into the fill border and flips
    some samples — otherwise the geometry test would not exercise them."""
    aug = _aug(8, pad=2, seed=11)
    dy, dx, flip = aug.params_at(0, 5, (8, 8))
    assert bool(((dy != 2) | (dx != 2)).any())
    assert bool(flip.any()) and not bool(flip.all())


def test_eval_is_centre_crop_and_leaves_the_counter():
    aug = _aug(8, pad=0, fill=3, **CIFAR)
    src = _batch(3, 10, 12)
    got = aug(src, train=False)
    assert aug.state_dict()["step"] == 0
    assert _same(got, _independent(aug, src, 0, train=False))
    # the centre crop, un-flipped, sample by sample
    scale = torch.tensor(aug.scale, dtype=torch.float64)
    bias = torch.tensor(aug.bias, dtype=torch.float64)
    want = (src[:, 1:9, 2:10].double() * scale + bias).float().bfloat16()
    assert _same(got, want)


def test_out_argument_is_filled_and_returned():
    aug = _aug(8, pad=2)
    src = _batch(2, 8, 8)
    out = torch.zeros(2, 8, 8, 3, dtype=torch.bfloat16)
    assert aug(src, out=out) is out
    assert _same(out, _independent(aug, src, 0))


def test_state_dict_round_trip():
    aug = _aug(8, pad=2, seed=5, **CIFAR)
    batches = [_batch(4, 8, 8, seed=s) for s in range(4)]
    outs = [aug(b) for b in batches]
    assert aug.state_dict() == {"seed": 5, "step": 4}
    fresh = _aug(8, pad=2, seed=99, **CIFAR)
    fresh.load_state_dict({"seed": 5, "step": 2})
    assert _same(fresh(batches[2]), outs[2])
    assert _same(fresh(batches[3]), outs[3])
    assert fresh.state_dict() == aug.state_dict()


def test_registers_as_stateful():
    from flashy_amd.state import StateManager, StateDictSource
    aug = _aug(8, pad=2, seed=5)
    assert isinstance(aug, StateDictSource)
    mgr = StateManager()
    mgr.register("augment", aug)
    aug(_batch(2, 8, 8))
    state = mgr.state_dict()
    assert state == {"augment": {"seed": 5, "step": 1}}
    other = _aug(8, pad=2)
    mgr2 = StateManager()
    mgr2.register("augment", other)
    mgr2.load_state_dict(state)
    assert other.state_dict() == {"seed": 5, "step": 1}


def test_argument_validation():
    aug = _aug(8, pad=2)
    good = _batch(2, 8, 8)
    with pytest.raises(TypeError, match="uint8"):
        aug(good.float())
    with pytest.raises(ValueError, match=r"\(2, 3, 8, 8\)"):
        aug(good.permute(0, 3, 1, 2).contiguous())            # NCHW
    with pytest.raises(ValueError, match="contiguous"):
        aug(_batch(2, 8, 16)[:, :, ::2])
    with pytest.raises(ValueError, match=r"\(2, 8, 8, 4\)"):
        aug(torch.zeros(2, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"exceeds the padded source \(7, 7\)"):
        aug(_batch(2, 3, 3))                                   # 3 + 2*2 < 8
    with pytest.raises(ValueError, match="exceeds"):
        aug.params_at(0, 2, (3, 3))
    with pytest.raises(TypeError, match="bfloat16"):
        aug(good, out=torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match=r"\(2, 8, 8, 3\)"):
        aug(good, out=torch.zeros(2, 6, 8, 3, dtype=torch.bfloat16))
    for bad in (dict(pad=-1), dict(flip=1.5), dict(mean=(0., 0.)),
                dict(std=(1., 0., 1.)), dict(fill=256)):
        with pytest.raises(ValueError):
            _aug(8, **bad)
    with pytest.raises(ValueError):
        _aug((8, 0))


# -- the example ------------------------------------------------------------

def test_synthetic_cifar_uint8_option():
    from examples.cifar.solver import SyntheticCIFAR
    f32, label = SyntheticCIFAR(4)[3]
    u8, label8 = SyntheticCIFAR(4, uint8=True)[3]
    assert label8 == label
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (32, 32, 3)
    want = (f32 * 64 + 128).round().clamp(0, 255).to(torch.uint8)
    assert torch.equal(u8, want.permute(1, 2, 0))
    again, _ = SyntheticCIFAR(4, uint8=True)[3]
    assert torch.equal(u8, again)


def _run_cifar(tmp: Path, *args: str) -> None:
    env = dict(os.environ)
    env["_FLASHY_AMD_DIR"] = str(tmp)
    env["PYTHONPATH"] = str(REPO) + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    subprocess.run(
        [sys.executable, "-m", "flashy_amd.run", "examples.cifar", *args,
         "run.exclude=[epochs,device,use_graph]", "device=cpu",
         "dataset_size=32", "valid_size=16", "batch_size=16",
         "augment.enabled=true"],
        check=True, cwd=REPO, env=env, timeout=300)


def _xp_dir(tmp: Path) -> Path:
    xps = list((tmp / "xps").iterdir())
    assert len(xps) == 1, xps
    return xps[0]


def test_cifar_example_with_augment_trains_and_resumes(tmp_path):
    _run_cifar(tmp_path, "--clear", "epochs=1")
    xp = _xp_dir(tmp_path)
    with open(xp / "history.json") as fh:
        hist = json.load(fh)
    assert len(hist) == 1
    assert math.isfinite(hist[0]["train"]["loss"])
    assert math.isfinite(hist[0]["valid"]["loss"])
    state = torch.load(xp / "checkpoint.th", weights_only=False)
    # 32 samples / batch 16 = 2 train batches; valid draws nothing
    assert state["augment"] == {"seed": 1234, "step": 2}

    _run_cifar(tmp_path, "epochs=2")
    with open(xp / "history.json") as fh:
        hist2 = json.load(fh)
    assert len(hist2) == 2 and hist2[:1] == hist
    state = torch.load(xp / "checkpoint.th", weights_only=False)
    assert state["augment"] == {"seed": 1234, "step": 4}
