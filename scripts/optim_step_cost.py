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

With ``--groups`` it times the per-tensor path instead, on an arena cut into
ResNet-50's own tensors (shapes from ``flashy_amd.models.resnet50``):

  plain        k_fused_sgd, one weight decay for every element
  no_decay_1d  k_fused_sgd_seg through the chunk table, BN / bias exempt
  lars         + k_seg_sqsum + k_lars_prepare: the full LARS step

Run on the GPU: PYTHONPATH=. python scripts/optim_step_cost.py [--groups]
"""
import argparse
import statistics

import torch

import flashy_amd.ops as ops
from flashy_amd.optim import LARS, FusedSGD, WarmupCosine, no_decay_1d

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


def r50_shapes():
    from flashy_amd.models import resnet50
    return [tuple(p.shape) for p in resnet50(num_classes=1000).parameters()]


def time_alternating(timed, rounds, iters):
    for fn in timed.values():       # warm every shape the windows use
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    results = {name: [] for name in timed}
    for _ in range(rounds):         # alternate, so drift hits all alike
        for name, fn in timed.items():
            results[name].append(window_us(fn, iters))
    return results


def groups_main(args):
    shapes = r50_shapes()
    n = sum(torch.Size(s).numel() for s in shapes)

    def make(**kw):
        params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02)
                  for s in shapes]
        opt = FusedSGD(params, lr=0.1, momentum=0.9, weight_decay=5e-4,
                       bf16_mirror=True, **kw)
        opt.grad_buffers[0].normal_(std=1e-3)
        return opt

    configs = {
        "plain": make(),
        "no_decay_1d": make(param_options=no_decay_1d),
        "lars": make(param_options=no_decay_1d, lars=LARS()),
    }
    assert configs["plain"].groups[0].seg is None
    table = configs["lars"].groups[0].seg
    group = configs["lars"].groups[0]
    timed = {name: opt.step for name, opt in configs.items()}
    timed["k_seg_sqsum alone"] = lambda: ops.seg_sqsum(
        group.flat_p, group.flat_g, table, group.seg_partials)
    results = time_alternating(timed, args.rounds, args.iters)

    print(f"arena: {n} floats in {len(shapes)} tensors, {table.n_chunks} "
          f"chunks of <= {ops.SEG_CHUNK}; {args.rounds} rounds x "
          f"{args.iters} steps")
    print(f"{'config':<20} {'median us':>10} {'min':>8} {'max':>8} "
          f"{'vs plain':>9}")
    t_plain = statistics.median(results["plain"])
    for name, ts in results.items():
        med = statistics.median(ts)
        print(f"{name:<20} {med:>10.1f} {min(ts):>8.1f} {max(ts):>8.1f} "
              f"{med / t_plain:>9.3f}")
    # bytes the algorithm needs: 22 per element for the update (p, g, m in;
    # p, m, bf16 p out), 16 per chunk for the table; 8 per element for norms
    t_seg = statistics.median(results["no_decay_1d"])
    t_norm = statistics.median(results["k_seg_sqsum alone"])
    print(f"plain:       {22 * n / 1e6:.1f} MB in {t_plain:.1f} us = "
          f"{22 * n / t_plain / 1e6:.2f} TB/s")
    print(f"no_decay_1d: {(22 * n + 16 * table.n_chunks) / 1e6:.1f} MB in "
          f"{t_seg:.1f} us = "
          f"{(22 * n + 16 * table.n_chunks) / t_seg / 1e6:.2f} TB/s")
    print(f"k_seg_sqsum: {8 * n / 1e6:.1f} MB in {t_norm:.1f} us = "
          f"{8 * n / t_norm / 1e6:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=R50_PARAMS)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--groups", action="store_true",
                    help="time the per-tensor / LARS path instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU timing says nothing here")
    torch.manual_seed(0)
    if args.groups:
        groups_main(args)
        return
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

    results = time_alternating(timed, args.rounds, args.iters)

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
