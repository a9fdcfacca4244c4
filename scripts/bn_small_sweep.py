# Time the single-kernel BatchNorm forms against the existing chain, per shape,
# in a hot loop (no tracing).  Each candidate is forced through the ops
# wrappers (ops.bn_fwd_small / ops.bn_bwd_small), whatever bn_small_plan says.
#   forward  chain = bn_finalize + bn_apply          small = k_bn_fwd_small
#   backward chain = bn_bwd_reduce + bn_bwd_grads + bn_bwd_apply
#            small = every form in ops.BN_BWD_SMALL_FORMS that runs the shape
# The loop is ITERS back-to-back repetitions captured into one HIP graph and
# replayed, because that is how the flagship runs them: a launch costs what it
# costs under replay, not what the Python caller costs.  "+res" rows add the
# residual operand forward and the dz write backward.
#   python scripts/bn_small_sweep.py             the table, then the plan's picks
#   python scripts/bn_small_sweep.py --passes 2  the whole table twice
import sys

import torch

sys.path.insert(0, ".")
from flashy_amd import ops  # noqa: E402

SHAPES = [  # (M, C)
    (1024, 512), (4096, 256),                   # ResNet-18/CIFAR layer4, layer3
    (4096, 1024), (1024, 2048), (3136, 2048),   # ResNet-50 (CIFAR, 224 px)
    (16384, 128),                               # layer2: the expected loser
    (256, 64), (512, 512), (4096, 64), (8192, 256),   # corners of the plan
]
ITERS = 50
REPLAYS = 20


def time_us(fn):
    """us per call of fn, ITERS calls per graph, best of REPLAYS replays."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(ITERS):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(REPLAYS):
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        graph.replay()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) / ITERS * 1000)
    return best


def run_shape(M, C):
    dev = "cuda"
    x = torch.randn(M, C, device=dev).to(torch.bfloat16)
    res = torch.randn(M, C, device=dev).to(torch.bfloat16)
    dy = torch.randn(M, C, device=dev).to(torch.bfloat16)
    y, dz, dx = (torch.empty_like(x) for _ in range(3))
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dgamma, dbeta = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    work = torch.empty(4 * C, device=dev)
    bsums = torch.empty(2 * C, device=dev)
    msplit = ops.bn_msplit(M, C)
    partials = torch.empty(msplit * 2 * C, device=dev)
    bpart = torch.empty(msplit * 2 * C, device=dev)
    ops.bn_stats(x, partials, M, C, msplit)

    def fwd_chain(r):
        ops.bn_finalize(partials, msplit, gamma, beta, rm, rv, work, M, C,
                        1e-5, 0.1, True)
        ops.bn_apply(x, r, y, work, M, C, True, 0.0)

    def fwd_small(r):
        ops.bn_fwd_small(partials, msplit, gamma, beta, rm, rv, work, x, r, y,
                         M, C, 1e-5, 0.1, True, True, 0.0)

    def bwd_chain():
        ops.bn_bwd_reduce(dy, y, x, work, dz, bpart, M, C, msplit, True, 0.0)
        ops.bn_bwd_grads(bpart, msplit, bsums, dgamma, dbeta, C)
        ops.bn_bwd_apply(dz, x, work, bsums, dx, M, C)

    def bwd_small(form, write_dz):
        ops.bn_bwd_small(dy, y, x, work, dz, dgamma, dbeta, dx, M, C, True,
                         0.0, write_dz=write_dz, form=form)

    fwd_chain(None)
    out = [f"M={M} C={C} plan={ops.bn_small_plan(M, C)}"]
    for tag, r in (("fwd", None), ("fwd+res", res)):
        out.append(f"  {tag}: chain {time_us(lambda: fwd_chain(r)):.2f}  "
                   f"small {time_us(lambda: fwd_small(r)):.2f}")
    for tag, wdz in (("bwd", False), ("bwd+res", True)):
        row = [f"chain {time_us(bwd_chain):.2f}"]
        for form in ops.BN_BWD_SMALL_FORMS:
            if form == "chain":
                continue
            try:
                bwd_small(form, wdz)
            except ValueError:      # the form cannot run this M
                row.append(f"{form} -")
                continue
            row.append(
                f"{form} {time_us(lambda: bwd_small(form, wdz)):.2f}")
        out.append(f"  {tag}: " + "  ".join(row))
    print("\n".join(out) + "   (us per BatchNorm)", flush=True)


if __name__ == "__main__":
    passes = int(sys.argv[sys.argv.index("--passes") + 1]) \
        if "--passes" in sys.argv else 1
    for p in range(passes):
        print(f"# pass {p + 1}", flush=True)
        for M, C in SHAPES:
            run_shape(M, C)
