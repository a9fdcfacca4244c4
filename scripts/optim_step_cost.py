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

With ``--lamb`` it times LAMB against Adam on the same arena, both with
``no_decay_1d`` and a bf16 mirror:

  adam_seg     k_fused_adam_seg: 7.5 words per element
  lamb         k_lamb_moments_seg + k_lamb_ratio + k_lamb_apply_seg: 10.5

and the two LAMB passes alone.  The five fp32 / bf16 buffers of the step are
460 MB, larger than the 256 MB last-level cache.

Run on the GPU: PYTHONPATH=. python scripts/optim_step_cost.py
                [--groups | --lamb]
"""
import argparse
import statistics

import torch

import flashy_amd.ops as ops
from flashy_amd.optim import (LARS, FusedAdam, FusedLAMB, FusedSGD,
                              WarmupCosine, no_decay_1d)

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


def lamb_main(args):
    shapes = r50_shapes()
    n = sum(torch.Size(s).numel() for s in shapes)

    def make(klass, **kw):
        params = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02)
                  for s in shapes]
        opt = klass(params, lr=1e-3, weight_decay=1e-2, bf16_mirror=True,
                    param_options=no_decay_1d, **kw)
        opt.grad_buffers[0].normal_(std=1e-3)
        return opt

    adam, lamb = make(FusedAdam, adamw=True), make(FusedLAMB)
    assert adam.groups[0].seg is not None
    # the passes alone run on a buffer set of their own, so the timed
    # optimizers stay independent of them
    alone = make(FusedLAMB)
    group, table = alone.groups[0], alone.groups[0].seg
    m, v = alone._exp_avg[0], alone._exp_avg_sq[0]
    step_dev = alone._step_dev[group.device]
    # pass 2 alone would repeat one ratio on moving weights, which need not
    # be stable; a ratio of 0 moves the same bytes and leaves p where it is
    no_step = torch.zeros_like(group.ratio)
    timed = {
        "adam_seg": adam.step,
        "lamb": lamb.step,
        "k_lamb_moments_seg alone": lambda: ops.lamb_moments(
            group.flat_p, group.flat_g, m, v, 0.9, 0.999, 1e-6, 0, table,
            group.seg_partials, step_dev=step_dev),
        "k_lamb_apply_seg alone": lambda: ops.lamb_apply(
            group.flat_p, m, v, 1e-3, 0.9, 0.999, 1e-6, 0, table, no_step,
            p_bf16=group.flat_p16, step_dev=step_dev),
    }
    results = time_alternating(timed, args.rounds, args.iters)
    assert torch.isfinite(lamb.groups[0].flat_p).all()

    print(f"arena: {n} floats in {len(shapes)} tensors, {table.n_chunks} "
          f"chunks of <= {ops.SEG_CHUNK}; {args.rounds} rounds x "
          f"{args.iters} steps")
    print(f"{'config':<26} {'median us':>10} {'min':>8} {'max':>8} "
          f"{'vs adam':>8} {'TB/s':>6}")
    # bytes the algorithm needs per element: Adam p g m v in, p m v bf16 out;
    # LAMB pass 1 p g m v in, m v out; pass 2 p m v in, p bf16 out
    words = {"adam_seg": 7.5, "lamb": 10.5, "k_lamb_moments_seg alone": 6.0,
             "k_lamb_apply_seg alone": 4.5}
    t_adam = statistics.median(results["adam_seg"])
    for name, ts in results.items():
        med = statistics.median(ts)
        print(f"{name:<26} {med:>10.1f} {min(ts):>8.1f} {max(ts):>8.1f} "
              f"{med / t_adam:>8.3f} {4 * words[name] * n / med / 1e6:>6.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=R50_PARAMS)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--groups", action="store_true",
                    help="time the per-tensor / LARS path instead")
    ap.add_argument("--lamb", action="store_true",
                    help="time FusedLAMB against segmented FusedAdam instead")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a CPU timing says nothing here")
    torch.manual_seed(0)
    if args.groups:
        groups_main(args)
        return
    if args.lamb:
        lamb_main(args)
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
