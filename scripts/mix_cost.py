# Copyright (c) Flashy-AMD authors.
"""Cost of the batch-mixing kernels (csrc/mix.hip) against the torch
composite doing the same work in place on the same bf16 NHWC tensor.

kernel    : k_batch_mix alone on a hand-written row (ops.batch_mix).
composite : mixup   x.mul_(lam).add_(x.flip(0) * (1 - lam))
            cutmix  box = x[:, y0:y1, x0:x1]; box.copy_(box.flip(0))
mixer     : DeviceMix(x, target): draw + mix + counter bump (3 launches),
            alpha = 1, rows drawn from the advancing counter.

Every case is captured REPS times into one graph, so the figures are kernel
time without launch gaps; medians over `--rounds` rounds of `--iters`
replays, the cases alternating within a round.  Compulsory bytes: 2 B read
+ 2 B written per mixed element (all N*H*W*C for mixup; both boxes of every
pair for cutmix; for `mixer` on cutmix the mean over the rows that ran).

Run on a GPU:  PYTHONPATH=. python scripts/mix_cost.py [--json out.json]
"""
import argparse
import json
import statistics
import struct

import torch

import flashy_amd.ops as ops
from flashy_amd.data import DeviceMix

SHAPE = (64, 224, 224, 3)
REPS = 20
LAM = 0.3
BOX = (33, 191, 33, 191)       # 158 x 158: half the image area (lam = 0.5)


def timed(fn, iters):
    """Mean device microseconds of one fn() over `iters` enqueued calls."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def graphed(fn):
    """fn repeated REPS times in one captured graph; returns its replay."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            fn()
    return graph.replay


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--iters", type=int, default=50)
    parser.add_argument("--rounds", type=int, default=9)
    parser.add_argument("--json")
    args = parser.parse_args()
    assert torch.cuda.is_available(), "mix_cost.py needs a GPU"

    n, h, w, c = SHAPE
    x = torch.randn(SHAPE, device="cuda").bfloat16()
    target = torch.arange(n, device="cuda")
    y0, y1, x0, x1 = BOX
    bits = struct.unpack("i", struct.pack("f", LAM))[0]
    row_mixup = torch.tensor([1, 0, 0, 0, 0, bits, 0, 0], dtype=torch.int32,
                             device="cuda")
    row_cutmix = torch.tensor([2, y0, y1, x0, x1, bits, 0, 0],
                              dtype=torch.int32, device="cuda")
    mixers = {"mixup": DeviceMix(mixup_alpha=1.0, seed=0),
              "cutmix": DeviceMix(cutmix_alpha=1.0, seed=0)}

    def composite_mixup():
        x.mul_(LAM).add_(x.flip(0) * (1 - LAM))

    def composite_cutmix():
        box = x[:, y0:y1, x0:x1]
        box.copy_(box.flip(0))

    cases = {
        ("mixup", "kernel"): graphed(lambda: ops.batch_mix(x, row_mixup)),
        ("mixup", "composite"): graphed(composite_mixup),
        ("mixup", "mixer"): graphed(lambda: mixers["mixup"](x, target)),
        ("cutmix", "kernel"): graphed(lambda: ops.batch_mix(x, row_cutmix)),
        ("cutmix", "composite"): graphed(composite_cutmix),
        ("cutmix", "mixer"): graphed(lambda: mixers["cutmix"](x, target)),
    }
    first = mixers["cutmix"].step
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):
        for key, replay in cases.items():
            samples[key].append(timed(replay, args.iters) / REPS)
            x.normal_()     # repeated blending decays the values to zero

    full = 4 * n * h * w * c
    box = 4 * 2 * (n // 2) * (y1 - y0) * (x1 - x0) * c
    last = mixers["cutmix"].step
    drawn = [mixers["cutmix"].row_at(s, (h, w)) for s in range(first, last)]
    mean_box = statistics.mean(
        4 * 2 * (n // 2) * (r[2] - r[1]) * (r[4] - r[3]) * c for r in drawn)
    nbytes = {("mixup", "kernel"): full, ("mixup", "composite"): full,
              ("mixup", "mixer"): full, ("cutmix", "kernel"): box,
              ("cutmix", "composite"): box, ("cutmix", "mixer"): mean_box}
    out = {"shape": SHAPE, "lam": LAM, "box": BOX, "reps": REPS,
           "iters": args.iters, "rounds": args.rounds, "cases": []}
    print(f"{'case':<20}{'median us':>11}{'min':>9}{'max':>9}{'MB':>9}"
          f"{'GB/s':>9}")
    for key, vals in samples.items():
        med = statistics.median(vals)
        rate = nbytes[key] / med / 1e3
        print(f"{key[0] + ' ' + key[1]:<20}{med:>11.2f}{min(vals):>9.2f}"
              f"{max(vals):>9.2f}{nbytes[key] / 1e6:>9.2f}{rate:>9.0f}")
        out["cases"].append({"mode": key[0], "case": key[1], "median_us": med,
                             "min_us": min(vals), "max_us": max(vals),
                             "bytes": nbytes[key], "gb_per_s": rate})
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
