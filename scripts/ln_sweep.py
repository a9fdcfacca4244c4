# Time the LayerNorm / bias+GELU / scale+residual kernels
# (csrc/layernorm.hip) on ConvNeXt-B stage shapes at batch 64, in a hot loop
# (no tracing), against the torch ops a user would otherwise call on the same
# bf16 tensors (F.layer_norm, x + b -> F.gelu, res + s * (z + b) and their
# autograd backward), and print the bytes each call must move over its time.
#   python scripts/ln_sweep.py                 all shapes, one process each
#   python scripts/ln_sweep.py --shape ln128   one shape, in-process
# The ops.* calls are timed as the modules run them: a backward includes its
# workspace allocation and its combine.  Ours and torch's are timed in
# alternating windows of ITERS calls, WINDOWS each; the table holds the median
# and the spread (max - min) / median of the windows.  `set` is what one call
# touches: at or under the 256 MB of last-level cache a hot loop can keep it
# resident, so those rows are cache rates, not HBM rates.  Each shape runs in
# a child process under its own `timeout`; the first child that fails ends the
# sweep.
import statistics
import subprocess
import sys

HW = {"128": 56, "256": 28, "512": 14, "1024": 7}   # ConvNeXt-B stages
SHAPES = {}     # name: (family, M, C)
for width, side in HW.items():
    M, C = 64 * side * side, int(width)
    SHAPES[f"ln{C}"] = ("ln", M, C)
    SHAPES[f"gelu{4 * C}"] = ("gelu", M, 4 * C)
    SHAPES[f"sr{C}"] = ("sr", M, C)
ITERS = 200
WINDOWS = 3
CHILD_TIMEOUT = 150


def run_shape(name):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ".")
    from flashy_amd import ops

    def window_us(fn):
        s, e = torch.cuda.Event(True), torch.cuda.Event(True)
        s.record()
        for _ in range(ITERS):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / ITERS * 1000

    def time_pair(ours, theirs):
        for fn in (ours, theirs):
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(WINDOWS):
            a.append(window_us(ours))
            b.append(window_us(theirs))
        return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t))
                for t in (a, b)]

    family, M, C = SHAPES[name]
    torch.manual_seed(3)
    act = [torch.randn(M, C, device="cuda").to(torch.bfloat16) for _ in range(3)]
    x, dy, res = act
    par = [torch.randn(C, device="cuda") for _ in range(4)]
    gamma, beta, b, s = par
    out, dx = torch.empty_like(x), torch.empty_like(x)
    grads = [torch.zeros(C, device="cuda") for _ in range(3)]
    # torch's side: bf16 parameters, as a bf16 module would hold them
    xt = x.clone().requires_grad_()
    tg, tb, tbias, ts = (p.to(torch.bfloat16).requires_grad_() for p in par)
    A = x.numel() * 2       # bytes of one activation
    if family == "ln":
        stats = torch.empty(M, 2, device="cuda")
        ops.ln_fwd(x, gamma, beta, out, stats, 1e-6)
        yt = F.layer_norm(xt, (C,), tg, tb, 1e-6)
        leaves = (xt, tg, tb)
        runs = {"fwd": (lambda: ops.ln_fwd(x, gamma, beta, out, stats, 1e-6),
                        lambda: F.layer_norm(xt, (C,), tg, tb, 1e-6), 2 * A),
                "bwd": (lambda: ops.ln_bwd(dy, x, stats, gamma, dx, *grads[:2]),
                        None, 3 * A)}
    elif family == "gelu":
        yt = F.gelu(xt + tbias)
        leaves = (xt, tbias)
        runs = {"fwd": (lambda: ops.bias_gelu_fwd(x, b, out),
                        lambda: F.gelu(xt + tbias), 2 * A),
                "bwd": (lambda: ops.bias_gelu_bwd(dy, x, b, dx, grads[0]),
                        None, 3 * A)}
    else:
        yt = res + ts * (xt + tbias)
        leaves = (xt, ts, tbias)
        runs = {"fwd": (lambda: ops.scale_residual_fwd(x, b, s, res, out),
                        lambda: res + ts * (xt + tbias), 3 * A),
                "bwd": (lambda: ops.scale_residual_bwd(dy, x, b, s, dx,
                                                       *grads[:2]),
                        None, 3 * A)}

    def torch_bwd():
        return torch.autograd.grad(yt, leaves, dy, retain_graph=True)

    line = [f"{name} {M}x{C} set {3 * A / 2 ** 20:.0f} MB:"]
    for direction, (ours, theirs, nbytes) in runs.items():
        (a, sa), (t, st) = time_pair(ours, theirs or torch_bwd)
        line.append(f"{direction} {a:.1f} us +-{sa:.0%} (torch {t:.1f} "
                    f"+-{st:.0%}) {nbytes / a / 1e3:.0f} GB/s")
    print("  ".join(line), flush=True)


if __name__ == "__main__":
    if "--shape" in sys.argv:
        run_shape(sys.argv[sys.argv.index("--shape") + 1])
        sys.exit(0)
    for name in SHAPES:
        rc = subprocess.run(
            ["timeout", "-k", "10", str(CHILD_TIMEOUT), sys.executable,
             __file__, "--shape", name]).returncode
        if rc:
            print(f"{name}: exit status {rc}; sweep stopped", flush=True)
            sys.exit(rc)
