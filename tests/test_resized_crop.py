# Copyright (c) Flashy-AMD authors.
"""CPU tests of flashy_amd.data.DeviceResizedCrop: the integer draw (pinned
against literal boxes, checked for its invariants and its fallback), the
fixed-point bilinear resample against ``F.interpolate`` within a derived
quantization bound, the exhaustive rounding check that makes the GPU tests
bitwise, state round trips, argument validation, and the CIFAR example with
``augment.resized_crop`` through the real CLI."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch
from torch.nn import functional as F

from flashy_amd.data import DeviceAugment, DeviceResizedCrop

REPO = Path(__file__).resolve().parent.parent

IDENTITY = dict(mean=(0., 0., 0.), std=(1 / 255, 1 / 255, 1 / 255))
CIFAR = dict(mean=(0.4914, 0.4822, 0.4465), std=(0.2023, 0.1994, 0.2010))
IMAGENET = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
DEFAULT_RATIO = (3 / 4, 4 / 3)


def _aug(out_size, **kw):
    kw.setdefault("device", "cpu")
    return DeviceResizedCrop(out_size, **kw)


def _batch(n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# -- the draw ---------------------------------------------------------------

# (seed, step, H, W, scale, ratio, p_flip) -> (y0, x0, h, w, flip, fallback)
# of samples 0..3, computed once from the pseudocode in docs/kernels.md by a
# stand-alone snippet
BOX_TABLE = [
    ((0, 0, 16, 16, (0.08, 1.0), DEFAULT_RATIO, 0.5),
     [(5, 8, 9, 8, True, False), (5, 6, 7, 6, True, False),
      (3, 9, 6, 7, True, False), (0, 2, 16, 14, False, False)]),
    ((0, 1, 9, 11, (0.08, 1.0), DEFAULT_RATIO, 0.5),
     [(1, 2, 8, 8, True, False), (0, 3, 6, 6, False, False),
      (1, 1, 3, 3, True, False), (0, 1, 7, 9, False, False)]),
    ((1234, 7, 256, 256, (0.08, 1.0), DEFAULT_RATIO, 0.5),
     [(19, 97, 167, 153, True, False), (105, 164, 92, 70, False, False),
      (30, 19, 223, 185, True, False), (5, 1, 194, 202, False, False)]),
    ((1234, 1000, 40, 56, (0.25, 0.75), (0.5, 2.0), 0.25),
     [(1, 3, 37, 27, False, False), (7, 31, 29, 23, False, False),
      (5, 3, 27, 52, False, False), (4, 4, 34, 17, False, False)]),
    ((7, 3, 375, 500, (0.08, 1.0), DEFAULT_RATIO, 0.5),
     [(46, 38, 217, 217, False, False), (171, 95, 134, 152, False, False),
      (54, 47, 313, 356, False, False), (164, 101, 159, 203, True, False)]),
    ((2 ** 63 + 5, 2 ** 40, 40, 56, (0.08, 1.0), DEFAULT_RATIO, 0.5),
     [(7, 13, 27, 24, False, False), (1, 0, 37, 32, False, False),
      (4, 26, 27, 25, False, False), (0, 11, 36, 40, False, False)]),
    ((2 ** 64 - 1, 2 ** 40 + 3, 16, 16, (0.08, 1.0), DEFAULT_RATIO, 1.0),
     [(2, 0, 13, 16, True, False), (0, 4, 11, 10, True, False),
      (10, 6, 6, 7, True, False), (3, 7, 5, 6, True, False)]),
    ((2 ** 63 + 5, 2 ** 40, 8, 64, (0.9, 1.0), DEFAULT_RATIO, 0.5),
     [(0, 26, 8, 11, False, True)] * 4),
    ((2 ** 63 + 5, 2 ** 40, 64, 8, (0.9, 1.0), DEFAULT_RATIO, 0.5),
     [(26, 0, 11, 8, False, True)] * 4),
]


@pytest.mark.parametrize("key,want", BOX_TABLE)
def test_boxes_at_literal_table(key, want):
    seed, step, H, W, scale, ratio, p = key
    aug = _aug(8, scale=scale, ratio=ratio, flip=p, seed=seed)
    boxes, fallback = aug.boxes_at(step, 4, (H, W))
    assert boxes.dtype == torch.int64 and tuple(boxes.shape) == (4, 5)
    assert fallback.dtype == torch.bool and tuple(fallback.shape) == (4,)
    got = [(*row[:4], bool(row[4]), fb)
           for row, fb in zip(boxes.tolist(), fallback.tolist())]
    assert got == want


def test_first_hash_levels_are_device_augments():
    """One seed drives both classes: the flip of DeviceAugment hashes
    ``mix(h0 + G)``, which is try 0's ``a`` here — checked through the
    shared helpers rather than a copy of them."""
    from flashy_amd import data
    assert DeviceResizedCrop.__module__ == DeviceAugment.__module__
    key = data._mix((5 + data._GOLDEN * 4) & data._M64)
    h0 = data._mix((key + data._GOLDEN * 1) & data._M64)
    crop = DeviceAugment(8, pad=2, seed=5, device="cpu")
    dy, dx, _ = crop.params_at(3, 1, (8, 8))
    assert int(dy[0]) == ((h0 & 0xffffffff) * 5) >> 32
    assert int(dx[0]) == ((h0 >> 32) * 5) >> 32
    # and the resized crop's flip bit comes from the same h0
    aug = _aug(8, seed=5)
    want = (data._mix((h0 + data._GOLDEN * 21) & data._M64) >> 40) < (1 << 23)
    assert bool(aug.boxes_at(3, 1, (16, 16))[0][0, 4]) == want


def _draws(aug, size, steps=1024, n=64):
    rows = [aug.boxes_at(step, n, size) for step in range(steps)]
    return torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows])


_DRAW_CASES = {
    "16x16": (dict(scale=(0.08, 1.0)), (16, 16)),
    "40x56": (dict(scale=(0.08, 1.0)), (40, 56)),
    "40x56-narrow": (dict(scale=(0.25, 0.75), ratio=(0.5, 2.0)), (40, 56)),
}
_DRAW_CACHE = {}


def _cached_draws(name):
    if name not in _DRAW_CACHE:
        kw, size = _DRAW_CASES[name]
        _DRAW_CACHE[name] = _draws(_aug(8, seed=3, **kw), size)
    return _DRAW_CACHE[name]


@pytest.mark.parametrize("name", sorted(_DRAW_CASES))
def test_box_invariants_over_65536_draws(name):
    kw, (H, W) = _DRAW_CASES[name]
    s0, s1 = kw["scale"]
    r0, r1 = kw.get("ratio", DEFAULT_RATIO)
    boxes, fallback = _cached_draws(name)
    assert boxes.shape[0] == 65536
    y0, x0, h, w, flip = (boxes[:, k] for k in range(5))
    assert int(h.min()) >= 1 and int(h.max()) <= H
    assert int(w.min()) >= 1 and int(w.max()) <= W
    assert int(y0.min()) >= 0 and int((y0 + h).max()) <= H
    assert int(x0.min()) >= 0 and int((x0 + w).max()) <= W

    # An accepted draw is (w, h) = round(side * sqrt(r), side / sqrt(r)) with
    # side^2 / (H W) in [s0, s1] and r in [r0, r1]; the table entries are bin
    # midpoints, strictly inside the ranges.  Rounding to whole pixels moves
    # each side by at most 1/2, and that is all the bounds are widened by.
    keep = ~fallback
    hd, wd = h[keep].double(), w[keep].double()
    hi_h, hi_w = hd + 0.5, wd + 0.5
    lo_h, lo_w = hd - 0.5, wd - 0.5
    assert bool((hi_h * hi_w >= s0 * H * W).all())
    assert bool((lo_h.clamp(min=0) * lo_w.clamp(min=0) <= s1 * H * W).all())
    assert bool((hi_w / lo_h >= r0).all())
    assert bool((lo_w / hi_h <= r1).all())
    # the draw uses its range: areas and ratios reach towards both ends
    area = hd * wd / (H * W)
    assert float(area.min()) < s0 + 0.1 * (s1 - s0) + 1.0 / (H * W)
    assert float(area.max()) > s1 - 0.1 * (s1 - s0) - (H + W + 1.0) / (H * W)
    assert float((wd / hd).min()) < 1 < float((wd / hd).max())

    n = boxes.shape[0]
    z = abs(int(flip.sum()) - n / 2) / math.sqrt(n / 4)
    print(f"{name}: flip {z:.2f} sd, fallbacks {int(fallback.sum())}")
    assert z <= 5.0, z


def test_no_fallback_on_a_square_source():
    _, fallback = _cached_draws("16x16")
    assert fallback.numel() == 65536
    assert int(fallback.sum()) == 0


def test_fallback_is_the_centred_ratio_bound_box():
    """8 x 64 at scale >= 0.9: every try wants h >= sqrt(0.9 * 512 * 3/4)
    = 18.6 > 8 rows, so all ten are rejected; W/H = 8 > 4/3, so the box is
    H rows by round(8 * 4/3) = 11 columns, centred."""
    aug = _aug(8, scale=(0.9, 1.0), seed=1)
    for step in (0, 1, 77):
        boxes, fallback = aug.boxes_at(step, 64, (8, 64))
        assert bool(fallback.all())
        assert boxes[:, :4].tolist() == [[0, 26, 8, 11]] * 64
        assert 0 < int(boxes[:, 4].sum()) < 64       # flips still vary
    # the transposed source hits the other bound: 8 columns, 11 rows
    boxes, fallback = aug.boxes_at(0, 8, (64, 8))
    assert bool(fallback.all())
    assert boxes[:, :4].tolist() == [[26, 0, 11, 8]] * 8
    # a square source against ratio 1/2: needs w 6.4, h 12.7 of 9 rows;
    # W/H = 1 > 1/2, so 9 rows by (9 * 32768 + 32768) >> 16 = 5 columns
    aug = _aug(8, scale=(1.0, 1.0), ratio=(0.5, 0.5), seed=1)
    boxes, fallback = aug.boxes_at(0, 8, (9, 9))
    assert bool(fallback.all())
    assert boxes[:, :4].tolist() == [[0, 2, 9, 5]] * 8
    # W/H inside the ratio range: the fallback is the whole image.  At the
    # full area only r within about 1/1000 of W/H = 2 fits, a few of the
    # 1024 levels between 1 and 4, so most samples exhaust their tries.
    aug = _aug(8, scale=(1.0, 1.0), ratio=(1.0, 4.0), seed=1)
    boxes, fallback = aug.boxes_at(0, 64, (1000, 2000))
    assert int(fallback.sum()) > 32
    assert boxes[fallback][:, :4].tolist() == \
        [[0, 0, 1000, 2000]] * int(fallback.sum())


# -- geometry ---------------------------------------------------------------

def _independent(aug, src, step):
    """Crop each box, ``F.interpolate`` it, flip where drawn: float
    [N, OH, OW, 3] on the 0..255 scale."""
    n, H, W, _ = src.shape
    boxes, _ = aug.boxes_at(step, n, (H, W))
    rows = []
    for i in range(n):
        y0, x0, h, w, flip = boxes[i].tolist()
        crop = src[i, y0:y0 + h, x0:x0 + w].permute(2, 0, 1)[None].double()
        res = F.interpolate(crop, size=aug.out_size, mode="bilinear",
                            align_corners=False, antialias=False)
        res = res[0].permute(1, 2, 0)
        rows.append(res.flip(1) if flip else res)
    return torch.stack(rows)


GEOMETRY = [
    # n, (h, w), out, extra
    (16, (9, 11), (6, 7), {}),
    (16, (16, 16), 8, {}),
    # upscales tiny boxes: 1 % to 5 % of 64 pixels, sides of 1 and 2 pixels
    (32, (8, 8), 12, dict(scale=(0.01, 0.05))),
]


@pytest.mark.parametrize("n,size,out,extra", GEOMETRY)
def test_geometry_matches_interpolate(n, size, out, extra):
    aug = _aug(out, seed=11, **IDENTITY, **extra)
    ref = _aug(out, seed=11, **IDENTITY, **extra)
    OH, OW = aug.out_size
    # weights truncated to 8 bits: < 2^-8 per axis; the floor in step_y /
    # step_x drifts a coordinate by < OH * 2^-16 resp. OW * 2^-16 pixels;
    # each moves the result by at most that fraction of 255 levels.  Then
    # the output is rounded to bf16: half an ulp at 255 is 0.5.
    bound = 255 * (2 * 2.0 ** -8 + (OH + OW) * 2.0 ** -16) + 0.5
    narrow = False
    for step in range(3):
        src = _batch(n, *size, seed=step)
        got = aug(src)
        assert got.dtype == torch.bfloat16
        assert tuple(got.shape) == (n, OH, OW, 3)
        want = _independent(ref, src, step)
        worst = float((got.double() - want).abs().max())
        print(f"{size} -> {(OH, OW)} step {step}: worst {worst:.3f} "
              f"of {bound:.3f} levels")
        assert worst <= bound
        boxes, _ = ref.boxes_at(step, n, size)
        assert torch.equal(aug.last_boxes[:, :4].long(), boxes[:, :4])
        narrow = narrow or int(boxes[:, 3].min()) == 1 \
            or int(boxes[:, 2].min()) == 1
    assert aug.state_dict() == {"seed": 11, "step": 3}
    if size == (8, 8):
        assert narrow, "the upscale case is meant to include 1-pixel boxes"


def test_constant_image_gives_the_constant():
    for norm in (IDENTITY, CIFAR, IMAGENET):
        aug = _aug((6, 7), seed=2, **norm)
        for value in (0, 1, 127, 255):
            src = torch.full((5, 9, 11, 3), value, dtype=torch.uint8)
            scale = torch.tensor(aug.scale, dtype=torch.float64)
            bias = torch.tensor(aug.bias, dtype=torch.float64)
            want = (value * scale + bias).float().bfloat16()
            got = aug(src)
            assert _same(got, want.expand_as(got).contiguous())
            got = aug(src, train=False)
            assert _same(got, want.expand_as(got).contiguous())


def test_whole_image_box_at_the_source_size_is_the_source():
    """scale = (1, 1), ratio = (1, 1) on a square source draws the whole
    image; at out_size == source size every weight is zero."""
    src = _batch(6, 8, 8, seed=5)
    aug = _aug(8, scale=(1.0, 1.0), ratio=(1.0, 1.0), seed=4, **IDENTITY)
    boxes, fallback = aug.boxes_at(0, 6, (8, 8))
    assert boxes[:, :4].tolist() == [[0, 0, 8, 8]] * 6
    assert not bool(fallback.any())
    flip = boxes[:, 4].bool()
    assert bool(flip.any()) and not bool(flip.all())
    got = aug(src).float()
    want = torch.where(flip[:, None, None, None], src.flip(2), src).float()
    assert torch.equal(got, want)
    # eval with eval_crop = 1 is the identity too, never flipped
    aug = _aug(8, eval_crop=1.0, **IDENTITY)
    assert torch.equal(aug(src, train=False).float(), src.float())


def test_eval_is_the_centred_box_and_leaves_the_counter():
    aug = _aug(224, eval_crop=224 / 256, seed=9)
    src = torch.zeros(2, 256, 256, 3, dtype=torch.uint8)
    aug(src, train=False)
    assert aug.last_boxes.tolist() == [[16, 16, 224, 224, 0, 65536, 65536, 0]] * 2
    assert aug.step == 0 and aug.state_dict() == {"seed": 9, "step": 0}
    # Resize(256) + CenterCrop(224) on a square source: the centre 7/8
    src = _batch(2, 32, 32, seed=1)
    aug = _aug(28, eval_crop=224 / 256, **IDENTITY)
    assert torch.equal(aug(src, train=False).float(),
                       src[:, 2:30, 2:30].float())
    # a wide source: the box has the output's aspect
    aug = _aug((6, 8), eval_crop=1.0)
    aug(torch.zeros(1, 12, 40, 3, dtype=torch.uint8), train=False)
    assert aug.last_boxes[0, :5].tolist() == [0, 12, 12, 16, 0]
    aug = _aug((6, 8), eval_crop=0.5)
    aug(torch.zeros(1, 40, 12, 3, dtype=torch.uint8), train=False)
    # largest 8:6 box is 12 wide, 9 high; half of it, rounded: 6 x 5 (4.5
    # rounds up)
    assert aug.last_boxes[0, :5].tolist() == [17, 3, 5, 6, 0]
    assert aug.step == 0


# -- rounding ---------------------------------------------------------------

@pytest.mark.parametrize("norm", [IDENTITY, CIFAR, IMAGENET],
                         ids=["identity", "cifar", "imagenet"])
def test_host_rounding_equals_the_fused_multiply_add(norm):
    """The kernel rounds the exact ``acc * scale' + bias`` once to fp32
    (fmaf), the host path rounds it to fp64 first.  The product of two
    24-bit significands is exact in fp64, so the two differ only where the
    fp64 sum is inexact AND lands on an fp32 rounding midpoint.  For every
    accumulator 0 .. 255 * 65536 and every channel there is no such sum."""
    aug = _aug(8, **norm)
    top = 255 * 65536
    chunk = 1 << 22
    for c in range(3):
        scale = aug.scale[c] / 65536.0
        assert scale * 65536.0 == aug.scale[c]       # the power of two is exact
        bias = torch.tensor(aug.bias[c], dtype=torch.float64)
        for lo in range(0, top + 1, chunk):
            acc = torch.arange(lo, min(lo + chunk, top + 1),
                               dtype=torch.float64)
            prod = acc * scale                       # exact
            total = prod + bias
            # Knuth's two-sum: err is the exact rounding error of `total`
            virt = total - prod
            err = (prod - (total - virt)) + (bias - virt)
            # an fp32 midpoint has the 29 dropped significand bits 1000...0
            midpoint = (total.view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
            bad = int(((err != 0) & midpoint).sum())
            assert bad == 0, (c, lo, bad)
            # fp64 -> fp32 must not leave the normal range (the midpoint
            # pattern above assumes it)
            nz = total != 0
            assert float(total[nz].abs().min()) > 2.0 ** -126 \
                if bool(nz.any()) else True


# -- state, validation ------------------------------------------------------

def test_state_dict_round_trip():
    aug = _aug(8, seed=5, **CIFAR)
    batches = [_batch(4, 12, 12, seed=s) for s in range(4)]
    outs = [aug(b) for b in batches]
    assert aug.state_dict() == {"seed": 5, "step": 4}
    assert aug.step == 4
    fresh = _aug(8, seed=99, **CIFAR)
    fresh.load_state_dict({"seed": 5, "step": 2})
    assert _same(fresh(batches[2]), outs[2])
    assert _same(fresh(batches[3]), outs[3])
    assert fresh.state_dict() == aug.state_dict()
    assert not _same(outs[0], aug(batches[0]))       # step 4 draws anew


def test_registers_as_stateful():
    from flashy_amd.state import StateManager, StateDictSource
    aug = _aug(8, seed=5)
    assert isinstance(aug, StateDictSource)
    mgr = StateManager()
    mgr.register("augment", aug)
    aug(_batch(2, 8, 8))
    assert mgr.state_dict() == {"augment": {"seed": 5, "step": 1}}


def test_out_argument_is_filled_and_returned():
    aug, ref = _aug(8, seed=1), _aug(8, seed=1)
    src = _batch(2, 12, 12)
    out = torch.zeros(2, 8, 8, 3, dtype=torch.bfloat16)
    assert aug(src, out=out) is out
    assert _same(out, ref(src))


def test_argument_validation():
    aug = _aug(8)
    good = _batch(2, 8, 8)
    with pytest.raises(TypeError, match="uint8"):
        aug(good.float())
    with pytest.raises(ValueError, match=r"\(2, 3, 8, 8\)"):
        aug(good.permute(0, 3, 1, 2).contiguous())            # NCHW
    with pytest.raises(ValueError, match="contiguous"):
        aug(_batch(2, 8, 16)[:, :, ::2])
    with pytest.raises(ValueError, match=r"\(2, 8, 8, 4\)"):
        aug(torch.zeros(2, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(TypeError, match="bfloat16"):
        aug(good, out=torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match=r"\(2, 8, 8, 3\)"):
        aug(good, out=torch.zeros(2, 6, 8, 3, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="40000"):
        aug.boxes_at(0, 2, (40000, 8))
    assert aug.step == 0
    for bad, match in (
            (dict(scale=(0.0, 1.0)), r"\(0\.0, 1\.0\)"),
            (dict(scale=(0.5, 0.25)), r"\(0\.5, 0\.25\)"),
            (dict(scale=(0.5, 1.5)), r"\(0\.5, 1\.5\)"),
            (dict(ratio=(0.0, 1.0)), r"\(0\.0, 1\.0\)"),
            (dict(ratio=(2.0, 1.0)), r"\(2\.0, 1\.0\)"),
            (dict(eval_crop=0.0), "0.0"), (dict(eval_crop=1.5), "1.5"),
            (dict(flip=1.5), "1.5"), (dict(mean=(0., 0.)), "mean"),
            (dict(std=(1., 0., 1.)), "std")):
        with pytest.raises(ValueError, match=match):
            _aug(8, **bad)
    with pytest.raises(ValueError, match="out_size"):
        _aug((8, 0))


# -- the example ------------------------------------------------------------

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
         "augment.enabled=true", "augment.resized_crop.scale=[0.25,1.0]",
         "augment.resized_crop.ratio=[0.75,1.3333]"],
        check=True, cwd=REPO, env=env, timeout=300)


def test_cifar_example_with_resized_crop_trains_and_resumes(tmp_path):
    _run_cifar(tmp_path, "--clear", "epochs=1")
    xps = list((tmp_path / "xps").iterdir())
    assert len(xps) == 1, xps
    xp = xps[0]
    with open(xp / "history.json") as fh:
        hist = json.load(fh)
    assert len(hist) == 1
    assert math.isfinite(hist[0]["train"]["loss"])
    assert math.isfinite(hist[0]["valid"]["loss"])
    state = torch.load(xp / "checkpoint.th", weights_only=False)
    # 32 samples / batch 16 = 2 train batches; valid draws nothing
    assert state["augment"] == {"seed": 1234, "step": 2}
    # the overrides reached the solver and selected the resized crop: its
    # log names the class with the scale and ratio given on the command line
    log = (xp / "solver.log.0").read_text()
    assert "on-device ingest: DeviceResizedCrop(out_size=(32, 32), " \
        "scale=(0.25, 1.0), ratio=(0.75, 1.3333), " in log

    _run_cifar(tmp_path, "epochs=2")
    with open(xp / "history.json") as fh:
        hist2 = json.load(fh)
    assert len(hist2) == 2 and hist2[:1] == hist
    state = torch.load(xp / "checkpoint.th", weights_only=False)
    assert state["augment"] == {"seed": 1234, "step": 4}


def test_example_selects_the_class_from_the_config():
    from examples.cifar.solver import make_augment
    from flashy_amd.config import Config
    base = dict(enabled=True, pad=4, flip=0.5, mean=[0., 0., 0.],
                std=[1., 1., 1.])
    assert make_augment(Config.wrap(dict(base, enabled=False)), 1, "cpu") \
        is None
    assert isinstance(make_augment(Config.wrap(base), 1, "cpu"),
                      DeviceAugment)
    off = make_augment(Config.wrap(dict(base, resized_crop=False)), 1, "cpu")
    assert isinstance(off, DeviceAugment)
    on = make_augment(Config.wrap(dict(base, resized_crop=True)), 7, "cpu")
    assert isinstance(on, DeviceResizedCrop)
    assert on.scale_range == (0.08, 1.0) and on.seed == 7
    tuned = make_augment(Config.wrap(dict(
        base, resized_crop=dict(scale=[0.25, 1.0], ratio=[0.5, 2.0]))),
        1, "cpu")
    assert isinstance(tuned, DeviceResizedCrop)
    assert tuned.scale_range == (0.25, 1.0) and tuned.ratio == (0.5, 2.0)
    assert tuned.out_size == (32, 32)
