"""What do the on-device LR schedule and global-norm clipping cost per step?

Times ``FusedSGD.step()`` (momentum, bf16 mirror) on a ResNet-50-sized flat
arena (25.6 M floats) in four configurations:

  plain     no schedule, no clipping: one k_fused_sgd launch
  schedule  + k_optim_prepare (one block) + k_step_inc
  clip      + k_grad_sqsum (one extra read of the gradient arena) + prepare
  both

The configurations are timed in alternation over several rounds, with device
events around a window of many steps, so the round-to-round spread of each is
printed next to its median.  The norm kernel is also timed alone, and its
achieved bytes/s is the 4*n bytes it has to read over that time.

Run on the GPU: PYTHONPATH=. python scripts/optim_step_cost.py
"""
import argparse
import statistics

import torch

import flashy_amd.ops as ops
from flashy_amd.optim import FusedSGD, WarmupCosine

R50_PARAMS = 25_557_032


def window_us(fn, iters):
    start = torch.cuda.Event(True)
    end = torch.cuda.Event(True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=R50_PARAMS)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU timing says nothing here")
    torch.manual_seed(0)
    n = args.n

    def make(**kw):
        p = torch.nn.Parameter(torch.randn(n, device="cuda") * 0.02)
        opt = FusedSGD([p], lr=0.1, momentum=0.9, weight_decay=5e-4,
                       bf16_mirror=True, **kw)
        opt.grad_buffers[0].normal_(std=1e-3)
        return opt

    sched = WarmupCosine(500, 100_000)
    configs = {
        "plain": make(),
        "schedule": make(schedule=sched),
        "clip": make(max_grad_norm=1.0),
        "both": make(schedule=sched, max_grad_norm=1.0),
    }
    g = configs["clip"].grad_buffers[0]
    partials = torch.empty(ops.grad_sqsum_blocks(n), device="cuda")
    timed = {name: opt.step for name, opt in configs.items()}
    timed["k_grad_sqsum alone"] = lambda: ops.grad_sqsum(g, partials)

    for fn in timed.values():       # warm every shape the windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    results = {name: [] for name in timed}
    for _ in range(args.rounds):    # alternate, so drift hits all alike
        for name, fn in timed.items():
            results[name].append(window_us(fn, args.iters))

    print(f"arena: {n} floats ({4 * n / 1e6:.1f} MB per fp32 buffer), "
          f"{args.rounds} rounds x {args.iters} steps")
    print(f"{'config':<20} {'median us':>10} {'min':>8} {'max':>8}")
    for name, ts in results.items():
        print(f"{name:<20} {statistics.median(ts):>10.1f} {min(ts):>8.1f} "
              f"{max(ts):>8.1f}")
    t_norm = statistics.median(results["k_grad_sqsum alone"])
    print(f"k_grad_sqsum: {4 * n / 1e6:.1f} MB read in {t_norm:.1f} us = "
          f"{4 * n / t_norm / 1e6:.2f} TB/s")
    # k_fused_sgd moves p, g, m in and p, m, bf16 p out: 22 bytes / element
    t_plain = statistics.median(results["plain"])
    print(f"plain step: {22 * n / 1e6:.1f} MB moved in {t_plain:.1f} us = "
          f"{22 * n / t_plain / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
